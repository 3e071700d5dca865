// render_distort.hip -- depth distortion of a finished forward (Mip-NeRF 360's distortion loss as 2DGS and gsplat's `distloss` use
// it) and its gradient, for gfx950.
//
// Definition.  For one pixel, walk its tile's list front to back exactly as the blend forward (render_fwd.hip) and k_render_median
// do, T = 1 at the start:
//     power > 0                                  -> skip
//     alpha = min(0.99, opacity exp(power));  alpha < 1/255 -> skip
//     test_T = T (1 - alpha);  test_T < 1e-4     -> stop, not blended
//     otherwise blend: w_i = alpha_i T_i, then T = test_T
// Each blended layer has a mapped depth m_i = c0 + c1 z_i + c2 / z_i, z_i = GaussRec::depth (the per-Gaussian value the expected
// depth blends); the three coefficients are per call ("ndc": far / (far - near) (1 - near / z); "linear": m = z).  The distortion is
//     D = sum_i w_i sum_{j<i} w_j (m_i - m_j)^2  =  sum_i w_i (mt_i^2 A_{i-1} + M2_{i-1} - 2 mt_i M1_{i-1}),
// A, M1, M2 the running sums of w, w mt, w mt^2 and mt_i = m_i - m_ref with m_ref the mapped depth of the pixel's FIRST blended
// layer: D depends on differences only, so the shift changes nothing mathematically (and sum_i dD/dm_i = 0; m_ref is a constant of
// the pixel), but in float32 the unshifted moments cancel -- 2 % error on the "ndc" values of a dense cloud, 0.2 absolute on D <= 1.3
// with m = z around 1000 -- where the shifted ones hold 1e-10 / 3e-5.  A layer's bracket is a sum of squares; its
// float32 value is held at >= 0, so D >= 0 everywhere.
//     distortion [1,H,W] float32 : D; exactly 0 for a pixel with fewer than two blended layers, for an overflowed async view, P = 0
//     moments    [H,W,4] float32 : {A, M1, M2, m_ref} of the pixel, what the backward needs of the forward
//
// Gradient, g = dL/dD of the pixel, A, M1, M2 its totals:
//     q_i = dD/dw_i = mt_i^2 A - 2 mt_i M1 + M2          dD/dm_i = 2 w_i (mt_i A - M1)          sum_i w_i q_i = 2 D
//     dD/dalpha_i = T_i q_i - S_i / (1 - alpha_i),   S_i = sum_{k>i} w_k q_k = 2 D - sum_{k<=i} w_k q_k
// S_i is taken FRONT TO BACK, on the forward's own T sequence: the backward is the forward's walk again, bit for bit the same
// decisions (no T un-blended by division, no stop position to be told), and a pixel that has stopped is done.  alpha is
// differentiated as if unclamped (the colour path's convention); alpha = opacity G reaches mean2D, conic and opacity with the
// expressions and scalings of the blend backward's flush (render_bwd.hip), and dL/dz_i = g dD/dm_i (c1 - c2 / z_i^2) goes to the
// slot's free float, which the depth-mode per-Gaussian backward (k_gauss_bwd_depth) takes to the mean.
//
// A pass of its own behind the forward, as lr_render_alpha and lr_render_median: the hand-scheduled blend pair stays as it is.
// k_render_distort: the quadrant walk of tile_walk.h (shape, staging, cull and alpha arithmetic are there), 256 list entries per
// round, the value kept per staged entry the mapped depth m_i, formed once per entry: its T sequence is the forward's under both
// forward shapes.  Unlike the median pass it needs the 1e-4 stop.
// k_distort_bwd: one workgroup per tile over the whole list (as depth mode), the same walk written out (tile_walk.h says why), 128
// entries per round with dm/dz in the slopes plane and the emission index beside it, with the per-pixel terms above; the
// seven sums of a list entry (D dx, D dy, D dx^2, D dx dy, D dy^2, D, dz with D = opacity G dL/dalpha) are reduced over the 64
// pixels of a wave with the blend backward's lane swaps and row sums (wave_reduce.h), stored per wave in LDS and added in wave
// order by the flush, which writes ONE plain 48-byte GradRec per instance -- {mean2D x, y, conic a, b | conic c, opacity, 0, 0 | 0, dz, 0, 0} in the blend
// backward's units, exact zeros for an entry no pixel blended, every slot of every list position written.  No global float atomics:
// bit-repeatable.  It OVERWRITES inst_grad: it runs after the colour backward of the same forward state and before another forward
// reuses the buffers.
#include "common.h"
#include "tile_walk.h"
#include "wave_reduce.h"

namespace lr {

namespace {

constexpr int DST_BATCH = 256;          // forward: staged list entries per round (10 KB of LDS)
constexpr int DSB_BATCH = 128;          // backward: staged list entries per round (6.5 KB + 16 KB of per-wave accumulators)
constexpr int DSB_COLS = 8;             // sums per entry and wave: D dx, D dy, D dx^2, D dx dy, D dy^2, D, dz, -

// mapped depth of a layer; ONE definition, so that the backward forms the bits the forward formed (mt = 0 on the first layer)
__device__ __forceinline__ float dst_map(float c0, float c1, float c2, float z)
{
#pragma clang fp contract(off)
    return (c0 + c1 * z) + c2 / z;                                    // (z > 0.2 for every listed Gaussian: in_frustum)
}

template <bool STRICT>
__global__ void __launch_bounds__(WALK_THREADS)
k_render_distort(int W, int H, int gx, int num_tiles, int tile_map, const uint2* __restrict__ ranges,
                 const char* __restrict__ bin_base, const GaussRec* __restrict__ rec, const GeomHeader* __restrict__ hdr,
                 float c0, float c1, float c2, float* __restrict__ out_dist, float4* __restrict__ out_mom)
{
    __shared__ float4 s_q0[DST_BATCH];      // WalkPlanes; the value kept in s_q1[].z: mapped depth m
    __shared__ float4 s_q1[DST_BATCH];
    __shared__ float2 s_q3[DST_BATCH];
    __shared__ int s_wdone[WALK_WAVES];

    const int tile = blend_tile(tile_map, num_tiles);
    if (tile < 0) return;
    const QuadLane q = quad_lane(tile, gx, W, H);
    const TileList tl = tile_list(hdr, ranges, bin_base, tile);     // overflowed: empty, no distortion anywhere

    float T = 1.0f, A = 0.0f, M1 = 0.0f, M2 = 0.0f, D = 0.0f, mref = 0.0f;
    uint64_t done = __builtin_amdgcn_ballot_w64(!q.inside);           // pixels that have stopped (or lie outside the image)

    tile_walk<STRICT, DST_BATCH>(
        q, tl, rec, WalkPlanes{s_q0, s_q1, s_q3, s_wdone}, done,
        [&](int, uint32_t, float z) { return dst_map(c0, c1, c2, z); },
        [&](int, float m, float alpha, uint64_t use) {
            const float test_T = T * (1.0f - alpha);
            const uint64_t stop = use & __builtin_amdgcn_ballot_w64(test_T < 0.0001f);
            if (__builtin_amdgcn_inverse_ballot_w64(use & ~stop)) {
                const float wt = alpha * T;
                if (A == 0.0f) mref = m;                              // the first blended layer (every weight is > 0)
                const float mt = m - mref;
                const float qq = fmaxf(0.0f, __builtin_fmaf(mt, __builtin_fmaf(mt, A, -2.0f * M1), M2));
                D = __builtin_fmaf(wt, qq, D);
                const float wm = wt * mt;
                A += wt;
                M1 += wm;
                M2 = __builtin_fmaf(wm, mt, M2);
                T = test_T;
            }
            return stop;
        },
        [](int, float, uint64_t) {});

    if (q.inside) {
        const size_t pix = (size_t)q.py * W + q.px;
        out_dist[pix] = D;
        out_mom[pix] = make_float4(A, M1, M2, mref);
    }
}

// a view without a list to read (P = 0): zeros everywhere
__global__ void __launch_bounds__(256) k_distort_fill(long long n, float* __restrict__ out_dist, float4* __restrict__ out_mom)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        out_dist[i] = 0.0f;
        out_mom[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dst_zero_slot(float4* __restrict__ inst_grad, uint32_t e)
{
    float4* slot = inst_grad + 3 * (size_t)e;
    slot[0] = make_float4(0.f, 0.f, 0.f, 0.f); slot[1] = slot[0]; slot[2] = slot[0];
}

// Launch bounds: at most 128 VGPRs, so that with 22.6 KB of LDS four workgroups fit a CU (the issue's floor is two).
template <bool STRICT>
__global__ void __launch_bounds__(WALK_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_distort_bwd(int W, int H, int gx, int num_tiles, int tile_map, const uint2* __restrict__ ranges, char* __restrict__ bin_base,
              const GaussRec* __restrict__ rec, const GeomHeader* __restrict__ hdr, const float* __restrict__ dL_ddist,
              const float* __restrict__ dist, const float4* __restrict__ mom, float c0, float c1, float c2)
{
    __shared__ float4 s_q0[DSB_BATCH];      // x, y, Ap, Bp (x log2 e; strict: conic a, b)
    __shared__ float4 s_q1[DSB_BATCH];      // Cp (strict: conic c), opacity, mapped depth m, qmax
    __shared__ float4 s_q2[DSB_BATCH];      // -b/c, -b/a, dm/dz = c1 - c2 / z^2, -
    __shared__ uint32_t s_id[DSB_BATCH];    // emission index (instance slot) of each staged entry
    __shared__ float s_acc[DSB_BATCH][WALK_WAVES][DSB_COLS];   // every wave its own copy: plain stores, summed in wave order
    __shared__ int s_wdone[WALK_WAVES];

    const int tile = blend_tile(tile_map, num_tiles);
    if (tile < 0) return;
    if (hdr->overflow != 0u) return;                                 // async mode: an overflowed view contributes nothing
    const uint2 range = ranges[tile];
    const int total = (int)(range.y - range.x);
    if (total == 0) return;
    const QuadLane q = quad_lane(tile, gx, W, H);
    const int tid = q.tid, w = q.w, l = q.l, px = q.px, py = q.py;
    const bool inside = q.inside;
    const float pxf = q.pxf, pyf = q.pyf, bx0 = q.bx0, bx1 = q.bx1, by0 = q.by0, by1 = q.by1;

    const BinLayout BL = bin_layout((long long)hdr->bin_bound);
    const uint32_t* __restrict__ point_list = reinterpret_cast<const uint32_t*>(bin_base + BL.point_list) + range.x;
    const uint32_t* __restrict__ list_gid = reinterpret_cast<const uint32_t*>(bin_base + BL.list_gid) + range.x;
    float4* __restrict__ inst_grad = reinterpret_cast<float4*>(bin_base + BL.inst_grad);

    // the pixel: upstream, 2 D and the forward's totals; a pixel without an upstream adds exact zeros and is done from the start
    float g = 0.0f, D2 = 0.0f;
    float4 mo = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) {
        const size_t pix = (size_t)py * W + px;
        g = dL_ddist[pix];
        D2 = 2.0f * dist[pix];
        mo = mom[pix];
    }
    float T = 1.0f, C = 0.0f;                                         // C = sum_{k<=i} w_k q_k
    uint64_t done = __builtin_amdgcn_ballot_w64(!inside || g == 0.0f);
    bool wave_done = done == ~0ull;
    const float ddelx_dx = (float)(0.5 * W), ddely_dy = (float)(0.5 * H);    // the NDC scale of dL/dmean2D (render_bwd.hip)

    const int row = l >> 4;
    const int col_a = (row == 0) ? 0 : (row == 1) ? 2 : (row == 2) ? 1 : 3;  // reduce8: rows hold terms {0, 2, 1, 3}
    const bool row_leader = (l & 15) == 0;

    for (int base = 0; base < total; base += DSB_BATCH) {
        if (l == 0) s_wdone[w] = wave_done ? 1 : 0;
        lds_barrier();                                                // (previous round fully flushed)
        if (s_wdone[0] + s_wdone[1] + s_wdone[2] + s_wdone[3] == WALK_WAVES) {
            // every pixel of the tile has stopped: the rest of the list was blended by nobody, its slots read as zero
            for (int p = base + tid; p < total; p += WALK_THREADS) dst_zero_slot(inst_grad, point_list[p]);
            break;
        }
        const int cnt = min(DSB_BATCH, total - base);
        if (tid < cnt) {
            const uint32_t id = list_gid[base + tid];
            const float4* gr = reinterpret_cast<const float4*>(rec + id);
            const float4 a = gr[0], b = gr[1], c = gr[2];
            const float z = c.y, m = dst_map(c0, c1, c2, z);
            s_q0[tid] = STRICT ? make_float4(a.x, a.y, a.z, a.w) : make_float4(a.x, a.y, (-0.5f * LOG2E) * a.z, -LOG2E * a.w);
            s_q1[tid] = STRICT ? make_float4(b.x, b.y, m, c.z) : make_float4((-0.5f * LOG2E) * b.x, b.y, m, LOG2E * c.z);
            s_q2[tid] = make_float4(-a.w / b.x, -a.w / a.z, c1 - c2 / (z * z), 0.f);
            s_id[tid] = point_list[base + tid];
        }
        {
            float4* z4 = reinterpret_cast<float4*>(&s_acc[0][0][0]);
            const int n4 = cnt * (WALK_WAVES * DSB_COLS / 4);
            for (int i = tid; i < n4; i += WALK_THREADS) z4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        lds_barrier();

        if (!wave_done) {
            for (int sb = 0; sb < cnt; sb += 64) {
                bool hit = false;
                const int jl = sb + l;
                if (jl < cnt) {
                    const float4 a = s_q0[jl];
                    const float4 b = s_q1[jl];
                    const float4 r = s_q2[jl];
                    const float ca = STRICT ? a.z : -2.0f * a.z, cb = STRICT ? a.w : -a.w, cc = STRICT ? b.x : -2.0f * b.x;
                    hit = box_hit(a.x, a.y, ca, cb, cc, r.x, r.y, b.w, bx0, bx1, by0, by1);
                }
                uint64_t mask = __ballot(hit);
                while (mask) {
                    const int k = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const int j = sb + k;
                    const float4 a = s_q0[j];
                    const float4 b = s_q1[j];
                    const float dx = a.x - pxf, dy = a.y - pyf;
                    float r0, r1, power;
                    gauss_row<STRICT>(a.w, b.x, dy, r0, r1);
                    const float t = b.y * gauss_weight<STRICT>(a.z, a.w, b.x, r0, r1, dx, power);   // alpha before the 0.99 clamp
                    const float alpha_f = fminf(0.99f, t);
                    const float test_T = T * (1.0f - alpha_f);
                    // the forward's decisions, on the forward's values
                    const uint64_t use = ~done & __builtin_amdgcn_ballot_w64(power <= 0.0f) & __builtin_amdgcn_ballot_w64(alpha_f >= 1.0f / 255.0f);
                    const uint64_t stop = use & __builtin_amdgcn_ballot_w64(test_T < 0.0001f);
                    const uint64_t blend = use & ~stop;
                    done |= stop;
                    if (blend != 0ull) {
                        // a pixel that does not blend the entry takes it as a layer with alpha = 0: every term is an exact zero
                        const bool bl = __builtin_amdgcn_inverse_ballot_w64(blend);
                        const float tm = bl ? t : 0.0f;
                        const float alpha = fminf(0.99f, tm);
                        const float wt = alpha * T;
                        const float mt = b.z - mo.w;
                        const float q = __builtin_fmaf(mt, __builtin_fmaf(mt, mo.x, -2.0f * mo.y), mo.z);
                        C = __builtin_fmaf(wt, q, C);
                        const float rinv = __builtin_amdgcn_rcpf(1.0f - alpha);
                        const float dDda = __builtin_fmaf(T, q, -((D2 - C) * rinv));
                        const float dop = tm * (g * dDda);                                  // opacity x G x dL/dalpha
                        const float zt = (2.0f * wt) * (__builtin_fmaf(mt, mo.x, -mo.y) * g);   // dL/dm of the layer
                        T = bl ? test_T : T;
                        const float mx = dop * dx, my = dop * dy;
                        float ra = mx, rb = my * dy;
                        reduce8(ra, my, mx * dx, mx * dy, rb, dop, zt, 0.0f);
                        ra = row_sum(ra);
                        rb = row_sum(rb);
                        if (row_leader) {
                            float* dst = &s_acc[j][w][col_a];
                            dst[0] = ra;
                            dst[4] = rb;
                        }
                    }
                    if (done == ~0ull) break;
                }
                if (done == ~0ull) { wave_done = true; break; }
            }
        }
        lds_barrier();
        if (tid < cnt) {
            float a8[DSB_COLS];
#pragma unroll
            for (int k = 0; k < DSB_COLS; k++) {
                float v = s_acc[tid][0][k];
#pragma unroll
                for (int a = 1; a < WALK_WAVES; a++) v += s_acc[tid][a][k];                  // fixed order over the waves
                a8[k] = v;
            }
            // the factors that are constant per Gaussian, as the blend backward's flush applies them
            const float4 q0 = s_q0[tid], q1 = s_q1[tid];
            const float ca = STRICT ? q0.z : (-2.0f * LN2) * q0.z, cb = STRICT ? q0.w : -LN2 * q0.w,
                        cc = STRICT ? q1.x : (-2.0f * LN2) * q1.x, o = q1.y;
            const float sx = a8[0], sy = a8[1], h = -0.5f;
            const float dopac = o > 0.f ? a8[5] * __builtin_amdgcn_rcpf(o) : 0.f;
            float4* slot = inst_grad + 3 * (size_t)s_id[tid];
            slot[0] = make_float4((-ca * sx - cb * sy) * ddelx_dx, (-cc * sy - cb * sx) * ddely_dy, h * a8[2], h * a8[3]);
            slot[1] = make_float4(h * a8[4], dopac, 0.f, 0.f);
            slot[2] = make_float4(0.f, a8[6] * s_q2[tid].z, 0.f, 0.f);
        }
    }
}

}  // namespace

void launch_render_distort(int W, int H, int P, const GeomView& g, const ImgView& im, const char* bin_base, float c0, float c1,
                           float c2, float* out_distortion, float* out_moments, hipStream_t s)
{
    const TileGrid t = tile_grid(W, H);
    if (t.num_tiles <= 0) return;
    float4* mom = reinterpret_cast<float4*>(out_moments);
    if (P <= 0) {                                                     // the forward of an empty cloud wrote no header and no list
        const long long n = (long long)W * H;
        hipLaunchKernelGGL(k_distort_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, out_distortion, mom);
        return;
    }
    dispatch_strict([&](auto st) {
        hipLaunchKernelGGL((k_render_distort<st.value>), dim3(t.grid), dim3(WALK_THREADS), 0, s, W, H, t.gx, t.num_tiles, t.tile_map,
                           im.ranges, bin_base, g.rec, g.header, c0, c1, c2, out_distortion, mom);
    });
}

void launch_distort_bwd(int W, int H, int P, const GeomView& g, const ImgView& im, char* bin_base, const float* dL_ddistortion,
                        const float* distortion, const float* moments, float c0, float c1, float c2, hipStream_t s)
{
    const TileGrid t = tile_grid(W, H);
    if (P <= 0 || t.num_tiles <= 0) return;
    dispatch_strict([&](auto st) {
        hipLaunchKernelGGL((k_distort_bwd<st.value>), dim3(t.grid), dim3(WALK_THREADS), 0, s, W, H, t.gx, t.num_tiles, t.tile_map,
                           im.ranges, bin_base, g.rec, g.header, dL_ddistortion, distortion, reinterpret_cast<const float4*>(moments), c0,
                           c1, c2);
    });
}

}  // namespace lr
