// render_fwd_quad_body.h -- the body of the quadrant blend forward k_render_fwd (render_fwd.hip), included INSIDE the kernel with
// STRICT, PAIR, DEPTH, COLOR (its template arguments), CARRY (constexpr bool), the kernel's parameters and its LDS planes s_q0 ..
// s_q3, s_wdone, s_seg0 in scope.  Textual, as gauss_bwd_body.h is: a colour-free kernel holds the body twice (render_fwd.hip
// says why), and an inlined __device__ template changes the instruction stream of the kernels that hold it once.
// COLOR: out_color is written.  CARRY: the pixel state has the colour channels -- always with COLOR, and without it for the
// tiles whose list is cut into segments: their checkpoints and c_final hold the colour so far, which the backward's segment
// start reads (render_bwd.hip load_pixel).  Without CARRY a tile has one staging round and no segments.
    static_assert(CARRY || !COLOR, "a colour image needs the colour channels");

    const int tile = blend_tile(tile_map, num_tiles);
    if (tile < 0) return;
    const int tx = tile % gx, ty = tile / gx;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const int x0 = tx * TILE_X + (w & 1) * 8, y0 = ty * TILE_Y + (w >> 1) * 8;      // this wave's 8x8 quadrant
    const int px = x0 + (l & 7), py = y0 + (l >> 3);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;
    const float bx0 = (float)x0, bx1 = (float)(x0 + 7), by0 = (float)y0, by1 = (float)(y0 + 7);

    const uint2 range = ranges[tile];
    const int total = (int)(range.y - range.x);

    PixState<DEPTH, CARRY> A = pix_start<DEPTH, CARRY>();
    uint64_t done = __builtin_amdgcn_ballot_w64(!inside);             // lane mask of finished pixels (all 64 lanes are live)
    bool wave_done = done == ~0ull;

    // A list longer than BWD_SEG is cut into segments for the backward (common.h BinLayout::seg_list / ckpt): one atomic
    // reserves the tile's slots, the (tile, segment) pairs are listed, and at the top of every later staging round the
    // waves still blending leave {T, colour so far} of their pixels; the final colour goes to c_final at the end
    static_assert(BATCH == BWD_SEG, "a staging round of the forward is one segment of the backward");
    const int n_seg = total > 0 ? (total - 1) / BWD_SEG : 0;
    uint32_t seg0 = 0;
    int n_ck = 0;                                                     // checkpoints this wave has written (segments 1 .. n_ck)
    if (n_seg > 0) {
        if (tid == 0) { s_seg0 = atomicAdd(&hdr->n_seg, (uint32_t)n_seg); tile_seg0[tile] = s_seg0; }
        lds_barrier();
        seg0 = s_seg0;
        for (int g = 1 + tid; g <= n_seg; g += THREADS) seg_list[seg0 + g - 1] = make_uint2((uint32_t)tile, (uint32_t)g);
    }

    for (int base = 0; base < total; base += BATCH) {
        // all quadrants finished?  (also the barrier that protects the LDS planes of the previous batch)
        if (l == 0) s_wdone[w] = wave_done ? 1 : 0;
        lds_barrier();
        if (s_wdone[0] + s_wdone[1] + s_wdone[2] + s_wdone[3] == NWAVES) break;
        const int cnt = min(BATCH, total - base);
        if constexpr (CARRY) if (base > 0 && !wave_done) {            // (without the colour channels: one round, no segments)
            // every pixel of a wave that is done stopped in front of this position: the backward starts those from final_T
            ckpt[(size_t)(seg0 + n_ck) * TILE_PIX + tid] = make_float4(A.T, A.Cr, A.Cg, A.Cb);
            n_ck++;
        }
        if (tid < cnt) {
            const uint32_t id = list_gid[range.x + base + tid];               // the Gaussian of the list position (BinLayout::list_gid)
            const float4* g = reinterpret_cast<const float4*>(rec + id);
            const float4 a = g[0], b = g[1], c = g[2];
            // default: Ap, Bp, Cp and the cull threshold scaled by log2(e); strict: the conic and the threshold as they are
            s_q0[tid] = STRICT ? make_float4(a.x, a.y, a.z, a.w) : make_float4(a.x, a.y, (-0.5f * LOG2E) * a.z, -LOG2E * a.w);
            s_q1[tid] = STRICT ? make_float4(b.x, b.y, c.y, c.z) : make_float4((-0.5f * LOG2E) * b.x, b.y, c.y, LOG2E * c.z);
            s_q2[tid] = make_float4(b.z, b.w, c.x, 0.f);
            s_q3[tid] = make_float2(-a.w / b.x, -a.w / a.z);
        }
        lds_barrier();
        if (wave_done) continue;

        for (int sb = 0; sb < cnt; sb += 64) {
            // CULL: lane l tests staged Gaussian sb+l against this wave's 8x8 quadrant
            bool hit = false;
            {
                const int j = sb + l;
                if (j < cnt) {
                    const float4 a = s_q0[j];
                    const float4 b = s_q1[j];
                    const float2 r = s_q3[j];
                    const float ca = STRICT ? a.z : -2.0f * a.z, cb = STRICT ? a.w : -a.w, cc = STRICT ? b.x : -2.0f * b.x;   // conic (x log2 e, like qmax)
                    hit = box_hit(a.x, a.y, ca, cb, cc, r.x, r.y, b.w, bx0, bx1, by0, by1);
                    // the outcome is kept for the backward (common.h BinLayout::quad_hits): every position a pixel of this
                    // quadrant can have blended lies in a chunk this wave culled
                    quad_hits[4 * ((size_t)range.x + (size_t)(base + j)) + w] = hit ? 1 : 0;
                }
            }
            uint64_t mask = __ballot(hit);
            // BLEND: walk the candidates in list order (a non-candidate is exactly the reference's `continue`: no pixel of
            // the quadrant can reach alpha >= 1/255)
            if (PAIR && total >= PAIR_MIN_LIST) {
                while (mask) {
                    const int k0 = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const bool two = mask != 0ull;
                    const int k1 = two ? __ffsll((long long)mask) - 1 : k0;
                    mask &= mask - 1;                                                  // (0 & anything = 0)
                    const int j0 = sb + k0, j1 = sb + k1;
                    float4 a0 = s_q0[j0], a1 = s_q0[j1];
                    float4 b0 = s_q1[j0], b1 = s_q1[j1];
                    const float4 c0 = s_q2[j0], c1 = s_q2[j1];
                    // Both candidates' reads are in flight before any arithmetic, and both alphas exist before the first step of
                    // the recursion: the empty asm statements tie the two candidates' values together (left to itself the compiler
                    // finishes candidate 0 -- reads, exponent, step -- before it even issues the reads of candidate 1)
                    asm volatile("" : "+v"(a0.x), "+v"(a0.y), "+v"(a0.z), "+v"(a0.w), "+v"(b0.x), "+v"(a1.x), "+v"(a1.y), "+v"(a1.z), "+v"(a1.w), "+v"(b1.x));
                    float r00, r01, r10, r11, power0, power1;
                    gauss_row<STRICT>(a0.w, b0.x, a0.y - pyf, r00, r01);                        // common.h gauss_power
                    gauss_row<STRICT>(a1.w, b1.x, a1.y - pyf, r10, r11);
                    float alpha0 = fminf(0.99f, b0.y * gauss_weight<STRICT>(a0.z, a0.w, b0.x, r00, r01, a0.x - pxf, power0));
                    float alpha1 = fminf(0.99f, b1.y * gauss_weight<STRICT>(a1.z, a1.w, b1.x, r10, r11, a1.x - pxf, power1));
                    asm volatile("" : "+v"(alpha0), "+v"(alpha1), "+v"(power0), "+v"(power1));
                    fwd_step(A, done, alpha0, power0, ~0ull, c0.x, c0.y, c0.z, b0.z, (uint32_t)(base + j0));
                    fwd_step(A, done, alpha1, power1, two ? ~0ull : 0ull, c1.x, c1.y, c1.z, b1.z, (uint32_t)(base + j1));
                }
            } else
            while (mask) {
                const int k = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int j = sb + k;
                const float4 a = s_q0[j];
                const float4 b = s_q1[j];
                const float4 c = s_q2[j];
                const uint32_t pos0 = (uint32_t)(base + j);
                const float dy = a.y - pyf;
                float r0, r1;
                gauss_row<STRICT>(a.w, b.x, dy, r0, r1);                                        // common.h gauss_power
                fwd_pixel<STRICT, DEPTH, CARRY>(A, done, a.z, a.w, b.x, r0, r1, a.x - pxf, b.y, c.x, c.y, c.z, b.z, pos0);
            }
            if (done == ~0ull) { wave_done = true; break; }             // all 64 pixels are finished
        }
    }

    if (inside) {
        const size_t N = (size_t)W * H;
        const size_t pix = (size_t)py * W + px;
        final_T[pix] = A.T;
        n_contrib[pix] = __builtin_amdgcn_inverse_ballot_w64(done) ? A.last : (uint32_t)total;
        if constexpr (CARRY) {
            const float fr = A.Cr + A.T * bg[0], fg = A.Cg + A.T * bg[1], fb = A.Cb + A.T * bg[2];
            if constexpr (COLOR) {
                out_color[pix] = fr;
                out_color[N + pix] = fg;
                out_color[2 * N + pix] = fb;
            }
            // a segmented tile: the final colour once more, where the backward's later segments find it (they subtract a
            // checkpoint's colour-so-far from it: the colour still to come behind that position, background included)
            if (n_seg > 0) c_final[pix] = make_float4(fr, fg, fb, 0.f);
        }
        if constexpr (DEPTH) out_depth[pix] = (A.acc > 0.5f) ? A.D / A.acc : 0.0f;         // forward.cu:384-388
    }
