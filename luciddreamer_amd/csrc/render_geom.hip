// render_geom.hip -- depth distortion AND rendered normal map of a finished forward in ONE tile walk each way, for gfx950: the pair
// the multi-view step (lr_views_accumulate) runs for its two geometry regularisers, and lr_render_geometry / lr_geometry_backward.
//
// The definitions are render_distort.hip's and render_normals.hip's, word for word: the mapped depth m = c0 + c1 z + c2 / z, the
// shift by m_ref (the pixel's first blended layer), D >= 0, N = sum_i w_i n_i with n_i from gauss_normals [P,4] as k_gauss_normals
// writes it, the forward's skips, 0.99 clamp and 1e-4 stop.  Both side passes walk the same lists with the same T sequence, the
// same skips and the same stop, and their two gradient records fit one GradRec together: one walk carries both.
//
// k_render_geom: a tile_walk<STRICT, 256> caller as k_render_distort and k_render_normals; a round stages the mapped depth (the kept
// value) and the Gaussian's normal; a pixel keeps the five distortion sums and the three components of N, each updated with the
// expression of the separate pass, so that the outputs are the separate passes' bits.
//     distortion [1,H,W], moments [H,W,4] = {A, M1, M2, m_ref}, normals [3,H,W]; zeros for an overflowed async view and for P = 0
//
// k_geom_bwd: the shape of k_normals_bwd (a 256-thread workgroup per tile, a wave per quadrant, 128 entries per round, S_i of both
// terms FRONT TO BACK on the forward's own T sequence).  Upstreams: gD = dL/dD per pixel (an image, or -- the step's weight x mean(D)
// -- one scalar for every pixel) and gN = dL/dN [3,H,W]; either may be absent and then contributes nothing.  Per blended layer
//     dL/dalpha_i = gD (T_i q_i - (2 D - Cq_i) / (1 - alpha_i)) + (T_i c_i - (N.gN - Cc_i) / (1 - alpha_i)),   c_i = n_i . gN,
// the two contributions added per pixel before they are multiplied out, so an entry has TEN sums: D dx, D dy, D dx^2, D dx dy,
// D dy^2, D (D = opacity G dL/dalpha), dz, and the three components of sum w gN.  Eight go through reduce8 and two row sums; the
// last two share one half-wave swap (reduce2: rows 0, 1 hold partials of the ninth, rows 2, 3 of the tenth) and one row sum, whose
// four row partials take a column each: 12 columns x 4 waves x 128 entries x 4 B = 24 576 B of per-wave accumulators plus 7.5 KB
// of staging, five workgroups per CU by LDS.  The flush writes ONE plain 48-byte GradRec per instance --
//     {mean2D x, y, conic a, b | conic c, opacity, dn.x, dn.y | dn.z, dz, 0, 0}
// -- the colour floats carry dL/dn as k_normals_bwd's do, pad0 carries dL/dz as k_distort_bwd's does: the depth-mode per-Gaussian
// backward (k_gauss_bwd_depth, as it stands) with dL_dgauss_normal in the colour row's place takes both on.  Exact zeros for an
// entry no pixel blended, every slot of every list position written.  No global float atomics: bit-repeatable.  It OVERWRITES
// inst_grad (lr_distortion_backward's ordering rule).
#include "common.h"
#include "tile_walk.h"
#include "wave_reduce.h"

namespace lr {

namespace {

constexpr int GM_BATCH = 256;           // forward: staged list entries per round (10 KB + 4 KB of LDS)
constexpr int GMB_BATCH = 128;          // backward: staged list entries per round
constexpr int GMB_COLS = 12;            // sums per entry and wave: reduce8's eight, then the four row partials of the last two

// mapped depth of a layer: render_distort.hip's dst_map, the same expression under the same contraction rule, so that this file
// forms the bits that file forms (mt = 0 on the first layer)
__device__ __forceinline__ float geom_map(float c0, float c1, float c2, float z)
{
#pragma clang fp contract(off)
    return (c0 + c1 * z) + c2 / z;                                    // (z > 0.2 for every listed Gaussian: in_frustum)
}

// Two per-lane terms over the wave down to 16-lane rows: on return rows 0, 1 of the result hold partials of `a` (lane l < 32:
// a[l] + a[l + 32]) and rows 2, 3 those of `b`; a row_sum finishes the job.  Inline asm for reduce8's reason, with its wait states.
__device__ __forceinline__ float reduce2(float a, float b)
{
    asm volatile("s_nop 1\n\t"
                 "v_permlane32_swap_b32 %0, %1\n\t"
                 "s_nop 0\n\t"
                 "v_add_f32 %0, %0, %1\n\t"
                 "s_nop 1"                                  // a DPP read of %0 follows
                 : "+v"(a), "+v"(b));
    return a;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <bool STRICT>
__global__ void __launch_bounds__(WALK_THREADS)
k_render_geom(int W, int H, int gx, int num_tiles, int tile_map, const uint2* __restrict__ ranges,
              const char* __restrict__ bin_base, const GaussRec* __restrict__ rec, const GeomHeader* __restrict__ hdr,
              const float4* __restrict__ gauss_normals, float c0, float c1, float c2, float* __restrict__ out_dist,
              float4* __restrict__ out_mom, float* __restrict__ out_normals)
{
    __shared__ float4 s_q0[GM_BATCH];       // WalkPlanes; the value kept in s_q1[].z: mapped depth m
    __shared__ float4 s_q1[GM_BATCH];
    __shared__ float2 s_q3[GM_BATCH];
    __shared__ float4 s_n[GM_BATCH];        // n.xyz of each staged entry
    __shared__ int s_wdone[WALK_WAVES];

    const int tile = blend_tile(tile_map, num_tiles);
    if (tile < 0) return;
    const QuadLane q = quad_lane(tile, gx, W, H);
    const TileList tl = tile_list(hdr, ranges, bin_base, tile);     // overflowed: empty, zeros everywhere

    float T = 1.0f, A = 0.0f, M1 = 0.0f, M2 = 0.0f, D = 0.0f, mref = 0.0f, Nx = 0.0f, Ny = 0.0f, Nz = 0.0f;
    uint64_t done = __builtin_amdgcn_ballot_w64(!q.inside);           // pixels that have stopped (or lie outside the image)

    tile_walk<STRICT, GM_BATCH>(
        q, tl, rec, WalkPlanes{s_q0, s_q1, s_q3, s_wdone}, done,
        [&](int slot, uint32_t id, float z) {
            const float4 n = gauss_normals[id];
            s_n[slot] = make_float4(n.x, n.y, n.z, 0.f);
            return geom_map(c0, c1, c2, z);
        },
        [&](int j, float m, float alpha, uint64_t use) {
            const float test_T = T * (1.0f - alpha);
            const uint64_t stop = use & __builtin_amdgcn_ballot_w64(test_T < 0.0001f);
            if (__builtin_amdgcn_inverse_ballot_w64(use & ~stop)) {
                const float wt = alpha * T;
                const float4 n = s_n[j];
                if (A == 0.0f) mref = m;                              // the first blended layer (every weight is > 0)
                const float mt = m - mref;
                const float qq = fmaxf(0.0f, __builtin_fmaf(mt, __builtin_fmaf(mt, A, -2.0f * M1), M2));
                D = __builtin_fmaf(wt, qq, D);
                const float wm = wt * mt;
                A += wt;
                M1 += wm;
                M2 = __builtin_fmaf(wm, mt, M2);
                Nx = __builtin_fmaf(wt, n.x, Nx);
                Ny = __builtin_fmaf(wt, n.y, Ny);
                Nz = __builtin_fmaf(wt, n.z, Nz);
                T = test_T;
            }
            return stop;
        },
        [](int, float, uint64_t) {});

    if (q.inside) {
        const size_t hw = (size_t)W * H, pix = (size_t)q.py * W + q.px;
        out_dist[pix] = D;
        out_mom[pix] = make_float4(A, M1, M2, mref);
        out_normals[pix] = Nx;
        out_normals[hw + pix] = Ny;
        out_normals[2 * hw + pix] = Nz;
    }
}

// a view without a list to read (P = 0): zeros everywhere
__global__ void __launch_bounds__(256) k_geom_fill(long long n, float* __restrict__ out_dist, float4* __restrict__ out_mom,
                                                   float* __restrict__ out_normals)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        out_dist[i] = 0.0f;
        out_mom[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        out_normals[i] = 0.0f; out_normals[n + i] = 0.0f; out_normals[2 * n + i] = 0.0f;
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void gm_zero_slot(float4* __restrict__ inst_grad, uint32_t e)
{
    float4* slot = inst_grad + 3 * (size_t)e;
    slot[0] = make_float4(0.f, 0.f, 0.f, 0.f); slot[1] = slot[0]; slot[2] = slot[0];
}

// Launch bounds: at most 128 VGPRs, so that with 32 KB of LDS five workgroups fit a CU
// dL_ddist: the image of dL/dD, or NULL: dist_scalar for every pixel (0: no distortion term; dist / mom are not read then);
// dL_dnormals: the image of dL/dN, or NULL: no normal term (normals is not read then)
template <bool STRICT>
__global__ void __launch_bounds__(WALK_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_geom_bwd(int W, int H, int gx, int num_tiles, int tile_map, const uint2* __restrict__ ranges, char* __restrict__ bin_base,
           const GaussRec* __restrict__ rec, const GeomHeader* __restrict__ hdr, const float* __restrict__ dL_ddist,
           float dist_scalar, const float* __restrict__ dist, const float4* __restrict__ mom, float c0, float c1, float c2,
           const float* __restrict__ dL_dnormals, const float* __restrict__ normals, const float4* __restrict__ gauss_normals)
{
    __shared__ float4 s_q0[GMB_BATCH];      // x, y, Ap, Bp (x log2 e; strict: conic a, b)
    __shared__ float4 s_q1[GMB_BATCH];      // Cp (strict: conic c), opacity, mapped depth m, qmax
    __shared__ float4 s_q2[GMB_BATCH];      // -b/c, -b/a, dm/dz = c1 - c2 / z^2, n.z
    __shared__ float2 s_n[GMB_BATCH];       // n.x, n.y
    __shared__ uint32_t s_id[GMB_BATCH];    // emission index (instance slot) of each staged entry
    __shared__ __attribute__((aligned(16))) float s_acc[GMB_BATCH][WALK_WAVES][GMB_COLS];   // every wave its own copy: plain stores, summed in wave order
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

    // the pixel: the two upstreams, 2 D, the forward's totals and N.g; a pixel without an upstream adds exact zeros and is done
    // from the start
    float g = 0.0f, D2 = 0.0f, gX = 0.0f, gY = 0.0f, gZ = 0.0f, Ng = 0.0f;
    float4 mo = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) {
        const size_t hw = (size_t)W * H, pix = (size_t)py * W + px;
        g = dL_ddist != nullptr ? dL_ddist[pix] : dist_scalar;
        if (g != 0.0f) {
            D2 = 2.0f * dist[pix];
            mo = mom[pix];
        }
        if (dL_dnormals != nullptr) {
            gX = dL_dnormals[pix]; gY = dL_dnormals[hw + pix]; gZ = dL_dnormals[2 * hw + pix];
            if (gX != 0.0f || gY != 0.0f || gZ != 0.0f)
                Ng = __builtin_fmaf(normals[2 * hw + pix], gZ, __builtin_fmaf(normals[hw + pix], gY, normals[pix] * gX));
        }
    }
    float T = 1.0f, Cq = 0.0f, Cc = 0.0f;                             // sum_{k<=i} w_k q_k, sum_{k<=i} w_k c_k
    uint64_t done = __builtin_amdgcn_ballot_w64(!inside || (g == 0.0f && gX == 0.0f && gY == 0.0f && gZ == 0.0f));
    bool wave_done = done == ~0ull;
    const float ddelx_dx = (float)(0.5 * W), ddely_dy = (float)(0.5 * H);    // the NDC scale of dL/dmean2D (render_bwd.hip)

    const int row = l >> 4;
    const int col_a = (row == 0) ? 0 : (row == 1) ? 2 : (row == 2) ? 1 : 3;  // reduce8: rows hold terms {0, 2, 1, 3}
    const bool row_leader = (l & 15) == 0;

    for (int base = 0; base < total; base += GMB_BATCH) {
        if (l == 0) s_wdone[w] = wave_done ? 1 : 0;
        lds_barrier();                                                // (previous round fully flushed)
        if (s_wdone[0] + s_wdone[1] + s_wdone[2] + s_wdone[3] == WALK_WAVES) {
            // every pixel of the tile has stopped: the rest of the list was blended by nobody, its slots read as zero
            for (int p = base + tid; p < total; p += WALK_THREADS) gm_zero_slot(inst_grad, point_list[p]);
            break;
        }
        const int cnt = min(GMB_BATCH, total - base);
        if (tid < cnt) {
            const uint32_t id = list_gid[base + tid];
            const float4* gr = reinterpret_cast<const float4*>(rec + id);
            const float4 a = gr[0], b = gr[1], c = gr[2];
            const float4 n = gauss_normals[id];
            const float z = c.y, m = geom_map(c0, c1, c2, z);
            s_q0[tid] = STRICT ? make_float4(a.x, a.y, a.z, a.w) : make_float4(a.x, a.y, (-0.5f * LOG2E) * a.z, -LOG2E * a.w);
            s_q1[tid] = STRICT ? make_float4(b.x, b.y, m, c.z) : make_float4((-0.5f * LOG2E) * b.x, b.y, m, LOG2E * c.z);
            s_q2[tid] = make_float4(-a.w / b.x, -a.w / a.z, c1 - c2 / (z * z), n.z);
            s_n[tid] = make_float2(n.x, n.y);
            s_id[tid] = point_list[base + tid];
        }
        {
            float4* z4 = reinterpret_cast<float4*>(&s_acc[0][0][0]);
            const int n4 = cnt * (WALK_WAVES * GMB_COLS / 4);
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
                        const float nz = s_q2[j].w;
                        const float2 nn = s_n[j];
                        const float tm = bl ? t : 0.0f;
                        const float alpha = fminf(0.99f, tm);
                        const float wt = alpha * T;
                        const float mt = b.z - mo.w;
                        const float qd = __builtin_fmaf(mt, __builtin_fmaf(mt, mo.x, -2.0f * mo.y), mo.z);
                        const float c = __builtin_fmaf(nz, gZ, __builtin_fmaf(nn.y, gY, nn.x * gX));     // n . g
                        Cq = __builtin_fmaf(wt, qd, Cq);
                        Cc = __builtin_fmaf(wt, c, Cc);
                        const float rinv = __builtin_amdgcn_rcpf(1.0f - alpha);
                        const float dDda = __builtin_fmaf(T, qd, -((D2 - Cq) * rinv));
                        const float dNda = __builtin_fmaf(T, c, -((Ng - Cc) * rinv));
                        const float dop = tm * __builtin_fmaf(g, dDda, dNda);               // opacity x G x dL/dalpha, both terms
                        const float zt = (2.0f * wt) * (__builtin_fmaf(mt, mo.x, -mo.y) * g);   // dL/dm of the layer
                        T = bl ? test_T : T;
                        const float mx = dop * dx, my = dop * dy;
                        float ra = mx, rb = my * dy;
                        reduce8(ra, my, mx * dx, mx * dy, rb, dop, zt, wt * gX);
                        ra = row_sum(ra);
                        rb = row_sum(rb);
                        const float rc = row_sum(reduce2(wt * gY, wt * gZ));                // rows 0, 1: dn.y; rows 2, 3: dn.z
                        if (row_leader) {
                            float* dst = &s_acc[j][w][0];
                            dst[col_a] = ra;
                            dst[4 + col_a] = rb;
                            dst[8 + row] = rc;
                        }
                    }
                    if (done == ~0ull) break;
                }
                if (done == ~0ull) { wave_done = true; break; }
            }
        }
        lds_barrier();
        if (tid < cnt) {
            float a12[GMB_COLS];
#pragma unroll
            for (int k = 0; k < GMB_COLS; k++) {
                float v = s_acc[tid][0][k];
#pragma unroll
                for (int a = 1; a < WALK_WAVES; a++) v += s_acc[tid][a][k];                  // fixed order over the waves
                a12[k] = v;
            }
            const float dny = a12[8] + a12[9], dnz = a12[10] + a12[11];
            // the factors that are constant per Gaussian, as the blend backward's flush applies them
            const float4 q0 = s_q0[tid], q1 = s_q1[tid];
            const float ca = STRICT ? q0.z : (-2.0f * LN2) * q0.z, cb = STRICT ? q0.w : -LN2 * q0.w,
                        cc = STRICT ? q1.x : (-2.0f * LN2) * q1.x, o = q1.y;
            const float sx = a12[0], sy = a12[1], h = -0.5f;
            const float dopac = o > 0.f ? a12[5] * __builtin_amdgcn_rcpf(o) : 0.f;
            float4* slot = inst_grad + 3 * (size_t)s_id[tid];
            slot[0] = make_float4((-ca * sx - cb * sy) * ddelx_dx, (-cc * sy - cb * sx) * ddely_dy, h * a12[2], h * a12[3]);
            slot[1] = make_float4(h * a12[4], dopac, a12[7], dny);
            slot[2] = make_float4(dnz, a12[6] * s_q2[tid].z, 0.f, 0.f);
        }
    }
}

}  // namespace

void launch_render_geom(int W, int H, int P, const GeomView& g, const ImgView& im, const char* bin_base, const float* gauss_normals,
                        float c0, float c1, float c2, float* out_distortion, float* out_moments, float* out_normals, hipStream_t s)
{
    const TileGrid t = tile_grid(W, H);
    if (t.num_tiles <= 0) return;
    float4* mom = reinterpret_cast<float4*>(out_moments);
    if (P <= 0) {                                                     // the forward of an empty cloud wrote no header and no list
        const long long n = (long long)W * H;
        hipLaunchKernelGGL(k_geom_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, out_distortion, mom, out_normals);
        return;
    }
    dispatch_strict([&](auto st) {
        hipLaunchKernelGGL((k_render_geom<st.value>), dim3(t.grid), dim3(WALK_THREADS), 0, s, W, H, t.gx, t.num_tiles, t.tile_map,
                           im.ranges, bin_base, g.rec, g.header, reinterpret_cast<const float4*>(gauss_normals), c0, c1, c2,
                           out_distortion, mom, out_normals);
    });
}

void launch_geom_bwd(int W, int H, int P, const GeomView& g, const ImgView& im, char* bin_base, const float* dL_ddistortion,
                     float dist_scalar, const float* distortion, const float* moments, float c0, float c1, float c2,
                     const float* dL_dnormals, const float* normals, const float* gauss_normals, hipStream_t s)
{
    const TileGrid t = tile_grid(W, H);
    if (P <= 0 || t.num_tiles <= 0) return;
    dispatch_strict([&](auto st) {
        hipLaunchKernelGGL((k_geom_bwd<st.value>), dim3(t.grid), dim3(WALK_THREADS), 0, s, W, H, t.gx, t.num_tiles, t.tile_map,
                           im.ranges, bin_base, g.rec, g.header, dL_ddistortion, dist_scalar, distortion,
                           reinterpret_cast<const float4*>(moments), c0, c1, c2, dL_dnormals, normals,
                           reinterpret_cast<const float4*>(gauss_normals));
    });
}

}  // namespace lr
