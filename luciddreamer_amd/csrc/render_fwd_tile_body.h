// render_fwd_tile_body.h -- the one-wave-per-tile blend forward (render_fwd_tile) with the per-pixel state and step it is built
// from, and the parameter list of the blend-forward kernels.  Included inside namespace lr { namespace { by render_fwd.hip
// (k_render_fwd, k_render_fwd_tile) and by render_bwd.hip (k_render_bwd_tile_step, which runs a tile's forward and backward in
// one wave); needs common.h.  The comments of render_fwd.hip describe the design.
#pragma once

// Per-pixel state of the blend.  `last` is what the backward needs from the reference's n_contrib (forward.cu:349, 379:
// the 1-based list position of the last blended Gaussian): every list position below it is evaluated, everything from it
// on is skipped.  Here it is the 0-based position of the Gaussian that STOPPED the pixel (T would fall below 1e-4), or
// the list length for a pixel that never stopped.  The positions between the reference's value and this one hold only
// Gaussians this pixel skipped (alpha < 1/255 or power > 0), which the backward skips again by the same test on the same
// arithmetic, so the gradients are identical -- and the common step loses the two instructions that tracked it.
// DEPTH = false (launch_render_fwd without out_depth: a view whose depth image nobody reads): no D and acc, and the two
// instructions per step that carried them are gone; every other field goes through the same operations.
// COLOR = false (launch_render_fwd without out_color either: a view of a multi-view step driven by fixed upstream gradients,
// whose blended colour nobody reads -- the backward starts from final_T and n_contrib, a Gaussian's colour comes from its
// GaussRec): no Cr / Cg / Cb, and the weight, its select and the three FMAs of a step are gone as well; T, done and last go
// through the same operations in the same order.  Three channel sets: colour + depth, colour, neither (a step that reads depth
// keeps carrying colour).
template <bool DEPTH, bool COLOR = true> struct PixState { float T, Cr, Cg, Cb, D, acc; uint32_t last; };
template <> struct PixState<false, true> { float T, Cr, Cg, Cb; uint32_t last; };
template <> struct PixState<false, false> { float T; uint32_t last; };
template <bool DEPTH, bool COLOR = true> __device__ __forceinline__ PixState<DEPTH, COLOR> pix_start()
{
    static_assert(COLOR || !DEPTH, "the depth channel goes with the colour");
    if constexpr (DEPTH) return PixState<true, true>{ 1.0f, 0.f, 0.f, 0.f, 0.f, 0.000001f, 0u };
    else if constexpr (COLOR) return PixState<false, true>{ 1.0f, 0.f, 0.f, 0.f, 0u };
    else return PixState<false, false>{ 1.0f, 0u };
}
// One candidate for the 64 pixels of the wave.  The per-pixel predicates live in wave-uniform 64-bit lane masks
// (v_cmp writes them to an SGPR pair; they are combined on the scalar unit and fed back to v_cndmask through
// inverse_ballot at no VALU cost); `done` is the mask of finished pixels.
template <bool STRICT, bool DEPTH, bool COLOR>
__device__ __forceinline__ void fwd_pixel(PixState<DEPTH, COLOR>& p, uint64_t& done, const float qA, const float qB, const float qC,
                                          const float r0, const float r1,
                                          const float dx, const float op, const float cr, const float cg, const float cb,
                                          const float depth, const uint32_t pos0)
{
    float power;                                                      // log2(e) x the reference's power (staged coefficients)
    const float alpha = fminf(0.99f, op * gauss_weight<STRICT>(qA, qB, qC, r0, r1, dx, power));
    const float test_T = p.T * (1.0f - alpha);
    // reference order of tests (forward.cu:331-347): power > 0 -> skip; alpha < 1/255 -> skip;
    // T*(1-alpha) < 1e-4 -> pixel done (this Gaussian is NOT blended)
    const uint64_t pass = ~done & __builtin_amdgcn_ballot_w64(power <= 0.0f) & __builtin_amdgcn_ballot_w64(alpha >= 1.0f / 255.0f);
    const uint64_t low_T = __builtin_amdgcn_ballot_w64(test_T < 0.0001f);
    const uint64_t stop = pass & low_T;
    const bool use = __builtin_amdgcn_inverse_ballot_w64(pass & ~low_T);
    done |= stop;
    if constexpr (COLOR) {
        const float wgt = use ? alpha * p.T : 0.f;
        p.Cr += cr * wgt; p.Cg += cg * wgt; p.Cb += cb * wgt;
        if constexpr (DEPTH) { p.D += depth * wgt; p.acc += wgt; }
    }
    p.T = use ? test_T : p.T;
    if (stop != 0ull) {                                                 // rare: a pixel stops at most once
        asm volatile("");                                               // keep it a scalar branch (no selects in the common path)
        p.last = __builtin_amdgcn_inverse_ballot_w64(stop) ? pos0 : p.last;
    }
}

#define LR_FWD_PARAMS int W, int H, int gx, int num_tiles, int tile_map, const uint2* __restrict__ ranges,                      \
                  const uint32_t* __restrict__ point_list, const uint32_t* __restrict__ list_gid,                              \
                  const GaussRec* __restrict__ rec,                                                                            \
                  const float* __restrict__ bg, float* __restrict__ final_T, uint32_t* __restrict__ n_contrib,                 \
                  float* __restrict__ out_color, float* __restrict__ out_depth, uint8_t* __restrict__ quad_hits,               \
                  GeomHeader* __restrict__ hdr, uint2* __restrict__ seg_list, float4* __restrict__ ckpt,                       \
                  uint32_t* __restrict__ tile_seg0, float4* __restrict__ c_final
#define LR_FWD_PASS W, H, gx, num_tiles, tile_map, ranges, point_list, list_gid, rec, bg, final_T, n_contrib, out_color,       \
                  out_depth, quad_hits, hdr, seg_list, ckpt, tile_seg0, c_final

// The TILE shape of the forward: ONE wave64 per 16x16 tile, a lane owns FOUR pixels -- the same position (l & 7, l >> 3) in
// each of the tile's four 8x8 quadrants (the layout of render_bwd.hip's TILE shape).  A round stages 64 list entries, one per
// lane: the lane culls its own entry against the four quadrants from registers (the four outcomes leave as ONE 4-byte store
// for the backward), the wave walks the union of the four candidate masks, reads a candidate's fields once, and steps only the
// quadrants it hit (scalar branches on the mask bits).  What it is for: everything the 4-wave shape pays per candidate and
// QUADRANT that is not a pixel step -- three broadcast LDS reads (8 + 6 + 6 LDS cycles), the mask bookkeeping on the scalar
// unit, the row terms of the exponent -- is paid once per candidate and TILE (an instance reaches 2.33 of its tile's 4
// quadrants at C3); no barriers, no partner waves to wait for, 3 KB of LDS.  Same operations per pixel and candidate in the
// same order as the quadrant kernel: the same bits (tests/test_gpu_variants.py).
// COLOR and CARRY: as in render_fwd_quad.
// HAND (render_bwd.hip k_render_bwd_tile_step): the four pixels' final T and stop position are also handed on in registers, as
// the backward's load_pixel would read them back (hand_T[q], hand_last[q]: the values of the epilogue's stores; T = 0 and
// last = 0 for a pixel outside the image).
constexpr int TSTAGE = 64;
template <bool STRICT, bool DEPTH, bool COLOR, bool CARRY, bool HAND = false>
__device__ __forceinline__ void
render_fwd_tile(LR_FWD_PARAMS, float4* s_q0, float4* s_q1, float4* s_q2, float* hand_T = nullptr, uint32_t* hand_last = nullptr)
{
    static_assert(CARRY || !COLOR, "a colour image needs the colour channels");
    // TIGHT: colour and depth in the state, default mode -- 28 registers of pixel state and the longest exponent chain.  Left to
    // itself the compiler keeps loop-invariant addresses across the candidate loop and runs out of the 64 registers: 12 bytes of
    // scratch (the lane's checkpoint address, spilled in front of the rounds).  Three such values are formed where they are
    // used, from operands the optimiser cannot see through (as the quadrant boxes below are, for every instantiation): no
    // scratch, a shift per round more.  All three are needed (with two of them 12 to 24 bytes stay); the other instantiations
    // keep their code.
    constexpr bool TIGHT = DEPTH && !STRICT;

    const int tile = blend_tile(tile_map, num_tiles);
    if (tile < 0) return;
    const int tx = tile % gx, ty = tile / gx;
    const int l = threadIdx.x;
    const int x0 = tx * TILE_X, y0 = ty * TILE_Y;
    const int pxl = x0 + (l & 7), pyt = y0 + (l >> 3);                // the lane's pixel in quadrant 0; + 8 for the right / lower ones
    const float pxf[2] = { (float)pxl, (float)(pxl + 8) }, pyf[2] = { (float)pyt, (float)(pyt + 8) };

    const uint2 range = ranges[tile];
    const int total = (int)(range.y - range.x);

    PixState<DEPTH, CARRY> A[4];
    uint64_t done[4];
    bool inside[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        A[q] = pix_start<DEPTH, CARRY>();
        inside[q] = pxl + (q & 1) * 8 < W && pyt + (q >> 1) * 8 < H;
        done[q] = __builtin_amdgcn_ballot_w64(!inside[q]);
    }

    // list segments for the backward: as in k_render_fwd (one atomic per tile; a checkpoint per pixel every BWD_SEG positions)
    static_assert(BWD_SEG % TSTAGE == 0, "checkpoints fall on round boundaries");
    // (HAND without CARRY: the fused kernel has branched on the list's length already -- one segment, nothing to list)
    const int n_seg = (HAND && !CARRY) ? 0 : total > 0 ? (total - 1) / BWD_SEG : 0;
    uint32_t seg0 = 0;
    if (n_seg > 0) {
        if (l == 0) { seg0 = atomicAdd(&hdr->n_seg, (uint32_t)n_seg); tile_seg0[tile] = seg0; }
        seg0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg0);
        for (int g = 1 + l; g <= n_seg; g += 64) seg_list[seg0 + g - 1] = make_uint2((uint32_t)tile, (uint32_t)g);
    }

    // A round's records arrive through three dependent loads (list -> Gaussian id -> record), and a single-wave workgroup has no
    // partner to wait with: the first two are issued a round ahead and are in flight while this round's candidates are walked
    // (positions beyond the list's end re-read its last entry, never staged).  Fetching the records ahead as well -- into
    // registers: the compiler waits for them where they are issued; straight into a second set of LDS planes with
    // global_load_lds_dwordx4: correct, 6 instead of 7 waves per SIMD -- measured no faster (profiles/r05w_ab_fwd_tile.json).
    const uint32_t* __restrict__ lgid = list_gid + range.x;            // the Gaussian of every list position (BinLayout::list_gid)
    uint32_t id_next = total > 0 ? lgid[min(l, total - 1)] : 0u;
    for (int base = 0; base < total; base += TSTAGE) {
        if ((done[0] & done[1] & done[2] & done[3]) == ~0ull) break;
        const int cnt = min(TSTAGE, total - base);
        const uint32_t id = id_next;
        if (base + TSTAGE < total) id_next = lgid[min(base + TSTAGE + l, total - 1)];
        if constexpr (CARRY) if (base > 0 && base % BWD_SEG == 0) {   // (without the colour channels: no segments, no such round)
            // (a quadrant whose pixels are all done stopped in front of this position: the backward starts those from final_T)
            float4* ck = ckpt;
            if constexpr (TIGHT) asm volatile("" : "+s"(ck));               // (the lane's checkpoint address: formed here)
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (done[q] != ~0ull)
                    ck[(size_t)(seg0 + base / BWD_SEG - 1) * TILE_PIX + q * 64 + l] = make_float4(A[q].T, A[q].Cr, A[q].Cg, A[q].Cb);
        }
        bool hit[4] = { false, false, false, false };
        lds_barrier();                                                // (the previous round's reads are done: one wave, no waiting)
        if (l < cnt) {
            // the quadrants' boxes are formed here, per round, from tile coordinates the optimiser cannot see through: kept
            // across the candidate loop they are eight more live registers (the tile's corner is uniform, but float conversions
            // live in vector registers)
            int x0v = x0, y0v = y0;
            asm volatile("" : "+s"(x0v), "+s"(y0v));
            const float bx[2][2] = { { (float)x0v, (float)(x0v + 7) }, { (float)(x0v + 8), (float)(x0v + 15) } };
            const float by[2][2] = { { (float)y0v, (float)(y0v + 7) }, { (float)(y0v + 8), (float)(y0v + 15) } };
            const float4* g = reinterpret_cast<const float4*>(rec + id);
            const float4 a = g[0], b = g[1], c = g[2];
            const float4 q0 = STRICT ? make_float4(a.x, a.y, a.z, a.w) : make_float4(a.x, a.y, (-0.5f * LOG2E) * a.z, -LOG2E * a.w);
            const float4 q1 = STRICT ? make_float4(b.x, b.y, c.y, c.z) : make_float4((-0.5f * LOG2E) * b.x, b.y, c.y, LOG2E * c.z);
            int ls = l;
            if constexpr (TIGHT) asm volatile("" : "+v"(ls));               // (the three planes' store addresses: formed per round)
            s_q0[ls] = q0; s_q1[ls] = q1; s_q2[ls] = make_float4(b.z, b.w, c.x, 0.f);
            const float r_c = -a.w / b.x, r_a = -a.w / a.z;
            const float ca = STRICT ? q0.z : -2.0f * q0.z, cb = STRICT ? q0.w : -q0.w, cc = STRICT ? q1.x : -2.0f * q1.x;
#pragma unroll
            for (int q = 0; q < 4; q++)
                hit[q] = box_hit(q0.x, q0.y, ca, cb, cc, r_c, r_a, q1.w, bx[q & 1][0], bx[q & 1][1], by[q >> 1][0], by[q >> 1][1]);
            // the outcome per quadrant, kept for the backward (common.h BinLayout::quad_hits)
            reinterpret_cast<uint32_t*>(quad_hits)[(size_t)range.x + (size_t)(base + l)] =
                (hit[0] ? 1u : 0u) | (hit[1] ? 0x100u : 0u) | (hit[2] ? 0x10000u : 0u) | (hit[3] ? 0x1000000u : 0u);
        }
        uint64_t m[4];
#pragma unroll
        for (int q = 0; q < 4; q++) m[q] = done[q] == ~0ull ? 0ull : __ballot(hit[q]);
        uint64_t mask = (m[0] | m[1]) | (m[2] | m[3]);
        lds_barrier();
        while (mask) {
            const int k = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const float4 fa = s_q0[k];
            const float4 fb = s_q1[k];
            const float4 fc = s_q2[k];
            const uint32_t pos0 = (uint32_t)(base + k);
            const uint64_t bit = 1ull << k;
#pragma unroll
            for (int row = 0; row < 2; row++) {
                if (((m[2 * row] | m[2 * row + 1]) & bit) == 0ull) continue;
                float r0, r1;
                gauss_row<STRICT>(fa.w, fb.x, fa.y - pyf[row], r0, r1);                         // common.h gauss_power
#pragma unroll
                for (int col = 0; col < 2; col++) {
                    const int q = 2 * row + col;
                    if ((m[q] & bit) == 0ull) continue;
                    fwd_pixel<STRICT, DEPTH, CARRY>(A[q], done[q], fa.z, fa.w, fb.x, r0, r1, fa.x - pxf[col], fb.y, fc.x, fc.y, fc.z, fb.z, pos0);
                    if (done[q] == ~0ull) {                            // the quadrant is finished: its later candidates are nobody's
                        m[q] = 0ull;
                        mask &= (m[0] | m[1]) | (m[2] | m[3]);
                    }
                }
            }
        }
    }

    const size_t N = (size_t)W * H;
    int x0e = x0, y0e = y0;
    if constexpr (TIGHT) asm volatile("" : "+s"(x0e), "+s"(y0e));           // (the pixel coordinates of the epilogue: formed here)
    const int pxe = x0e + (l & 7), pye = y0e + (l >> 3);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if constexpr (HAND) {
            hand_T[q] = inside[q] ? A[q].T : 0.f;
            hand_last[q] = inside[q] ? (__builtin_amdgcn_inverse_ballot_w64(done[q]) ? A[q].last : (uint32_t)total) : 0u;
        }
        if (!inside[q]) continue;
        const int px = pxe + (q & 1) * 8, py = pye + (q >> 1) * 8;
        const size_t pix = (size_t)py * W + px;
        final_T[pix] = A[q].T;
        n_contrib[pix] = __builtin_amdgcn_inverse_ballot_w64(done[q]) ? A[q].last : (uint32_t)total;
        if constexpr (CARRY) {
            const float fr = A[q].Cr + A[q].T * bg[0], fg = A[q].Cg + A[q].T * bg[1], fb = A[q].Cb + A[q].T * bg[2];
            if constexpr (COLOR) {
                out_color[pix] = fr;
                out_color[N + pix] = fg;
                out_color[2 * N + pix] = fb;
            }
            if (n_seg > 0) c_final[pix] = make_float4(fr, fg, fb, 0.f);
        }
        if constexpr (DEPTH) out_depth[pix] = (A[q].acc > 0.5f) ? A[q].D / A[q].acc : 0.0f;         // forward.cu:384-388
    }
}
