// render_features.hip -- the N-channel feature map of a finished forward (semantic / instance logits, distilled 2D features,
// per-Gaussian appearance codes: what Feature-3DGS, LangSplat and LEGaussians blend, what gsplat renders for any channel count)
// and its gradient, for gfx950.
//
// Input.  features [P,C] float32, 1 <= C <= LR_FEATURE_MAX_CHANNELS, view-independent, used as given (no activation, raw mode
// included).
// Per-pixel map.  The walk of k_render_normals (tile_walk.h: the forward's skips, 0.99 clamp and 1e-4 stop, bit for bit its T
// sequence), w_i = alpha_i T_i:
//     out_features [C,H,W] float32 : F[c] = sum_i w_i f_i[c]; no background term, no normalisation; exact zeros for a pixel with
//                                    no layer, for P = 0 and for an overflowed async view
// The channels are taken FTR_K at a time, one walk per chunk: a lane keeps FTR_K accumulators in registers, a round stages
// f_i[c0 : c0 + FTR_K] of its entries in an LDS plane that the wave reads as float4 broadcasts.  Every channel is an fma chain of
// its own in list order: its bits do not depend on the chunk it sits in or on what else is in C.  The tail chunk is padded with
// zeros in LDS: nothing is read past column C, no plane >= C is written.
//
// Gradient, g = dL/dF of the pixel, c_i = f_i . g:
//     dL/df_i[c] += w_i g[c]      dL/dalpha_i = T_i c_i - S_i / (1 - alpha_i),   S_i = sum_{k>i} w_k c_k = F.g - sum_{k<=i} w_k c_k
// S_i is taken FRONT TO BACK on the forward's own T sequence, as k_normals_bwd takes it.  dL/dalpha is linear in g, so the chunks'
// parts add: a chunk works with its own channels' c_i and F.g alone.  The clamp is not differentiated; skips, stop and order are
// constants.  alpha = opacity G reaches mean2D, conic and opacity with the expressions of the blend backward's flush.
//
// k_features_bwd: the shape of k_normals_bwd with 6 + FTR_K sums per list entry and wave (D dx, D dy, D dx^2, D dx dy, D dy^2, D
// with D = opacity G dL/dalpha, then w g[c] per channel), eight at a time through reduce8 and two row sums, into per-wave LDS
// accumulators that the flush sums in wave order.  The geometric part goes to the instance's 48-byte GradRec in inst_grad (colour
// floats zero): the first chunk OVERWRITES the slot, a later chunk adds to it with a plain load / add / store (a slot belongs to
// one (tile, entry), so to one workgroup, and launches on one stream are ordered).  The feature part goes to workspace
// [slots][FTR_K] float32 by emission slot; every slot of every list position is written, zeros where nobody blended.
// k_feature_rows: per emitting Gaussian the sum of its contiguous workspace rows (the rank-ordered `offsets`, as gauss_bwd_body.h
// reads them, capped at num_sorted) into dL_dfeatures[i, c0 : c0 + FTR_K], serial for short ranges, a fixed-shape wave reduction
// for long ones.  No global float atomics anywhere: bit-repeatable.
#include "common.h"
#include "tile_walk.h"
#include "wave_reduce.h"

namespace lr {

namespace {

// (-DLR_FTR_K / -DLR_FTR_BWD_BATCH: the measured alternatives of DESIGN 4b-FTR; the product build defines neither)
#ifndef LR_FTR_K
constexpr int FTR_K = 16;               // channels per walk (how it was chosen)
#else
constexpr int FTR_K = LR_FTR_K;
#endif
constexpr int RF_BATCH = 256;           // forward: staged list entries per round (10 KB of planes + 16 KB of features at K = 16)
#ifndef LR_FTR_BWD_BATCH
constexpr int FB_BATCH = 64;            // backward: staged list entries per round
#else
constexpr int FB_BATCH = LR_FTR_BWD_BATCH;
#endif
constexpr int FB_GROUPS = (6 + FTR_K + 7) / 8;      // reduce8 calls per candidate
constexpr int FB_COLS = 8 * FB_GROUPS;              // sums per entry and wave, padded to whole groups
constexpr int FR_THREADS = 256;         // k_feature_rows
constexpr uint32_t FR_SERIAL_MAX = 24;  // instances summed by the owning lane; more -> the whole wave helps (as k_gauss_bwd)

static_assert(FTR_K % 4 == 0, "the feature plane is read and written as float4");

// the K floats of row `id` from column c0 on, zeros from column C on; vec: C % 4 == 0 and the base is 16-byte aligned
template <int K>
__device__ __forceinline__ void load_feature_chunk(const float* __restrict__ features, uint32_t id, int C, int c0, bool vec,
                                                   float4* __restrict__ dst)
{
    const float* row = features + (size_t)id * C + c0;
    const int left = C - c0;                                          // > 0
    if (vec) {
#pragma unroll
        for (int q = 0; q < K / 4; q++)
            dst[q] = 4 * q < left ? reinterpret_cast<const float4*>(row)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
        for (int q = 0; q < K / 4; q++) {
            float4 v;
            v.x = 4 * q + 0 < left ? row[4 * q + 0] : 0.f;
            v.y = 4 * q + 1 < left ? row[4 * q + 1] : 0.f;
            v.z = 4 * q + 2 < left ? row[4 * q + 2] : 0.f;
            v.w = 4 * q + 3 < left ? row[4 * q + 3] : 0.f;
            dst[q] = v;
        }
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <bool STRICT, int K>
__global__ void __launch_bounds__(WALK_THREADS)
k_render_features(int W, int H, int gx, int num_tiles, int tile_map, const uint2* __restrict__ ranges,
                  const char* __restrict__ bin_base, const GaussRec* __restrict__ rec, const GeomHeader* __restrict__ hdr,
                  const float* __restrict__ features, int C, int c0, int vec, float* __restrict__ out)
{
    __shared__ float4 s_q0[RF_BATCH];       // WalkPlanes; s_q1[].z is not used by this pass
    __shared__ float4 s_q1[RF_BATCH];
    __shared__ float2 s_q3[RF_BATCH];
    __shared__ float4 s_f[RF_BATCH][K / 4]; // f[c0 : c0 + K] of each staged entry
    __shared__ int s_wdone[WALK_WAVES];

    const int tile = blend_tile(tile_map, num_tiles);
    if (tile < 0) return;
    const QuadLane q = quad_lane(tile, gx, W, H);
    const TileList tl = tile_list(hdr, ranges, bin_base, tile);     // overflowed: empty, zeros everywhere

    float T = 1.0f;
    float acc[K];
#pragma unroll
    for (int c = 0; c < K; c++) acc[c] = 0.0f;
    uint64_t done = __builtin_amdgcn_ballot_w64(!q.inside);           // pixels that have stopped (or lie outside the image)

    tile_walk<STRICT, RF_BATCH>(
        q, tl, rec, WalkPlanes{s_q0, s_q1, s_q3, s_wdone}, done,
        [&](int slot, uint32_t id, float) {
            load_feature_chunk<K>(features, id, C, c0, vec != 0, s_f[slot]);
            return 0.0f;
        },
        [&](int j, float, float alpha, uint64_t use) {
            const float test_T = T * (1.0f - alpha);
            const uint64_t stop = use & __builtin_amdgcn_ballot_w64(test_T < 0.0001f);
            if (__builtin_amdgcn_inverse_ballot_w64(use & ~stop)) {
                const float wt = alpha * T;
#pragma unroll
                for (int q4 = 0; q4 < K / 4; q4++) {
                    const float4 f = s_f[j][q4];
                    acc[4 * q4 + 0] = __builtin_fmaf(wt, f.x, acc[4 * q4 + 0]);
                    acc[4 * q4 + 1] = __builtin_fmaf(wt, f.y, acc[4 * q4 + 1]);
                    acc[4 * q4 + 2] = __builtin_fmaf(wt, f.z, acc[4 * q4 + 2]);
                    acc[4 * q4 + 3] = __builtin_fmaf(wt, f.w, acc[4 * q4 + 3]);
                }
                T = test_T;
            }
            return stop;
        },
        [](int, float, uint64_t) {});

    if (q.inside) {
        const size_t hw = (size_t)W * H, pix = (size_t)q.py * W + q.px;
#pragma unroll
        for (int c = 0; c < K; c++)
            if (c0 + c < C) out[(size_t)(c0 + c) * hw + pix] = acc[c];
    }
}

// a view without a list to read (P = 0): zeros everywhere
__global__ void __launch_bounds__(256) k_features_fill(long long n, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 0.0f;
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// an entry no pixel blended: the slot reads as zero (first chunk only: a later chunk leaves what the first wrote), and so does
// its workspace row (every chunk; rows beyond the caller's workspace are not touched -- k_feature_rows reports them)
template <int K>
__device__ __forceinline__ void ftr_zero_entry(float4* __restrict__ inst_grad, float4* __restrict__ ws, uint32_t ws_slots, uint32_t e,
                                               bool first)
{
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (first) {
        float4* slot = inst_grad + 3 * (size_t)e;
        slot[0] = z; slot[1] = z; slot[2] = z;
    }
    if (e < ws_slots) {
        float4* r = ws + (size_t)e * (K / 4);
#pragma unroll
        for (int q = 0; q < K / 4; q++) r[q] = z;
    }
}

// Launch bounds: at most 128 VGPRs, so that with 32 KB of LDS five workgroups fit a CU
template <bool STRICT, int K>
__global__ void __launch_bounds__(WALK_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_features_bwd(int W, int H, int gx, int num_tiles, int tile_map, const uint2* __restrict__ ranges, char* __restrict__ bin_base,
               const GaussRec* __restrict__ rec, const GeomHeader* __restrict__ hdr, const float* __restrict__ dL_dout,
               const float* __restrict__ out_features, const float* __restrict__ features, int C, int c0, int vec,
               float4* __restrict__ ws, uint32_t ws_slots)
{
    __shared__ float4 s_q0[FB_BATCH];       // x, y, Ap, Bp (x log2 e; strict: conic a, b)
    __shared__ float4 s_q1[FB_BATCH];       // Cp (strict: conic c), opacity, -, qmax
    __shared__ float2 s_q2[FB_BATCH];       // -b/c, -b/a
    __shared__ float4 s_f[FB_BATCH][K / 4]; // f[c0 : c0 + K] of each staged entry
    __shared__ uint32_t s_id[FB_BATCH];     // emission index (instance slot) of each staged entry
    __shared__ __attribute__((aligned(16))) float s_acc[FB_BATCH][WALK_WAVES][FB_COLS];   // every wave its own copy: plain stores, summed in wave order
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
    const bool first = c0 == 0;

    const BinLayout BL = bin_layout((long long)hdr->bin_bound);
    const uint32_t* __restrict__ point_list = reinterpret_cast<const uint32_t*>(bin_base + BL.point_list) + range.x;
    const uint32_t* __restrict__ list_gid = reinterpret_cast<const uint32_t*>(bin_base + BL.list_gid) + range.x;
    float4* __restrict__ inst_grad = reinterpret_cast<float4*>(bin_base + BL.inst_grad);

    // the pixel: the chunk's upstream and its share of F.g; channels from C on read as zero
    float g[K];
    float Fg = 0.0f;
#pragma unroll
    for (int c = 0; c < K; c++) {
        g[c] = 0.0f;
        if (inside && c0 + c < C) {
            const size_t at = (size_t)(c0 + c) * ((size_t)W * H) + ((size_t)py * W + px);
            g[c] = dL_dout[at];
            Fg = __builtin_fmaf(out_features[at], g[c], Fg);
        }
    }
    float T = 1.0f, Csum = 0.0f;                                      // Csum = sum_{k<=i} w_k c_k
    // (a pixel whose upstream is zero is walked all the same: what is `done` must not depend on the chunk's other channels)
    uint64_t done = __builtin_amdgcn_ballot_w64(!inside);
    bool wave_done = done == ~0ull;
    const float ddelx_dx = (float)(0.5 * W), ddely_dy = (float)(0.5 * H);    // the NDC scale of dL/dmean2D (render_bwd.hip)

    const int row = l >> 4;
    const int col_a = (row == 0) ? 0 : (row == 1) ? 2 : (row == 2) ? 1 : 3;  // reduce8: rows hold terms {0, 2, 1, 3}
    const bool row_leader = (l & 15) == 0;

    for (int base = 0; base < total; base += FB_BATCH) {
        if (l == 0) s_wdone[w] = wave_done ? 1 : 0;
        lds_barrier();                                                // (previous round fully flushed)
        if (s_wdone[0] + s_wdone[1] + s_wdone[2] + s_wdone[3] == WALK_WAVES) {
            // every pixel of the tile has stopped: the rest of the list was blended by nobody
            for (int p = base + tid; p < total; p += WALK_THREADS) ftr_zero_entry<K>(inst_grad, ws, ws_slots, point_list[p], first);
            break;
        }
        const int cnt = min(FB_BATCH, total - base);
        if (tid < cnt) {
            const uint32_t id = list_gid[base + tid];
            const float4* gr = reinterpret_cast<const float4*>(rec + id);
            const float4 a = gr[0], b = gr[1], c = gr[2];
            s_q0[tid] = STRICT ? make_float4(a.x, a.y, a.z, a.w) : make_float4(a.x, a.y, (-0.5f * LOG2E) * a.z, -LOG2E * a.w);
            s_q1[tid] = STRICT ? make_float4(b.x, b.y, 0.f, c.z) : make_float4((-0.5f * LOG2E) * b.x, b.y, 0.f, LOG2E * c.z);
            s_q2[tid] = make_float2(-a.w / b.x, -a.w / a.z);
            s_id[tid] = point_list[base + tid];
            load_feature_chunk<K>(features, id, C, c0, vec != 0, s_f[tid]);
        }
        {
            float4* z4 = reinterpret_cast<float4*>(&s_acc[0][0][0]);
            const int n4 = cnt * (WALK_WAVES * FB_COLS / 4);
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
                    const float2 r = s_q2[jl];
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
                        float c = 0.0f;                                                      // f . g over the chunk
#pragma unroll
                        for (int q4 = 0; q4 < K / 4; q4++) {
                            const float4 f = s_f[j][q4];
                            c = __builtin_fmaf(f.x, g[4 * q4 + 0], c);
                            c = __builtin_fmaf(f.y, g[4 * q4 + 1], c);
                            c = __builtin_fmaf(f.z, g[4 * q4 + 2], c);
                            c = __builtin_fmaf(f.w, g[4 * q4 + 3], c);
                        }
                        Csum = __builtin_fmaf(wt, c, Csum);
                        const float rinv = __builtin_amdgcn_rcpf(1.0f - alpha);
                        const float dFda = __builtin_fmaf(T, c, -((Fg - Csum) * rinv));
                        const float dop = tm * dFda;                                        // opacity x G x dL/dalpha
                        T = bl ? test_T : T;
                        const float mx = dop * dx, my = dop * dy;
                        // term k of the entry: the six geometric ones, then w g[c]; zeros pad the last group
                        const auto term = [&](int k) {
                            return k == 0 ? mx : k == 1 ? my : k == 2 ? mx * dx : k == 3 ? mx * dy : k == 4 ? my * dy : k == 5 ? dop
                                 : k < 6 + K ? wt * g[k - 6 < K ? k - 6 : 0] : 0.0f;
                        };
                        float* dst = &s_acc[j][w][0];
#pragma unroll
                        for (int grp = 0; grp < FB_GROUPS; grp++) {
                            float ra = term(8 * grp), rb = term(8 * grp + 4);
                            reduce8(ra, term(8 * grp + 1), term(8 * grp + 2), term(8 * grp + 3),
                                    rb, term(8 * grp + 5), term(8 * grp + 6), term(8 * grp + 7));
                            ra = row_sum(ra);
                            rb = row_sum(rb);
                            if (row_leader) {
                                dst[8 * grp + col_a] = ra;
                                dst[8 * grp + 4 + col_a] = rb;
                            }
                        }
                    }
                    if (done == ~0ull) break;
                }
                if (done == ~0ull) { wave_done = true; break; }
            }
        }
        lds_barrier();
        if (tid < cnt) {
            const auto col = [&](int k) {
                float v = s_acc[tid][0][k];
#pragma unroll
                for (int wv = 1; wv < WALK_WAVES; wv++) v += s_acc[tid][wv][k];              // fixed order over the waves
                return v;
            };
            float a[6];
#pragma unroll
            for (int k = 0; k < 6; k++) a[k] = col(k);
            // the factors that are constant per Gaussian, as the blend backward's flush applies them
            const float4 q0 = s_q0[tid], q1 = s_q1[tid];
            const float ca = STRICT ? q0.z : (-2.0f * LN2) * q0.z, cb = STRICT ? q0.w : -LN2 * q0.w,
                        cc = STRICT ? q1.x : (-2.0f * LN2) * q1.x, o = q1.y;
            const float sx = a[0], sy = a[1], h = -0.5f;
            const float dopac = o > 0.f ? a[5] * __builtin_amdgcn_rcpf(o) : 0.f;
            const uint32_t e = s_id[tid];
            float4* slot = inst_grad + 3 * (size_t)e;
            float4 g0 = make_float4((-ca * sx - cb * sy) * ddelx_dx, (-cc * sy - cb * sx) * ddely_dy, h * a[2], h * a[3]);
            float4 g1 = make_float4(h * a[4], dopac, 0.f, 0.f);
            if (!first) {
                const float4 p0 = slot[0], p1 = slot[1];
                g0.x += p0.x; g0.y += p0.y; g0.z += p0.z; g0.w += p0.w;
                g1.x += p1.x; g1.y += p1.y;
                slot[0] = g0; slot[1] = g1;
            } else {
                slot[0] = g0; slot[1] = g1;
                slot[2] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            if (e < ws_slots) {
                float4* r = ws + (size_t)e * (K / 4);
#pragma unroll
                for (int q4 = 0; q4 < K / 4; q4++) r[q4] = make_float4(col(6 + 4 * q4), col(7 + 4 * q4), col(8 + 4 * q4), col(9 + 4 * q4));
            }
        }
    }
}

// every lane ends with the wave's total, the four row totals added in row order
__device__ __forceinline__ float ftr_wave_sum(float v)
{
    v = row_sum(v);
    return ((__shfl(v, 0) + __shfl(v, 16)) + __shfl(v, 32)) + __shfl(v, 48);
}

// One lane per emitting Gaussian (rank t of vis_list): the sum of its workspace rows into dL_dfeatures[idx, c0 : c0 + K].
// accumulate: added to what is there, else written (the caller zero-filled the rows of the Gaussians that emit nothing).
template <int K>
__global__ void __launch_bounds__(FR_THREADS)
k_feature_rows(GeomHeader* __restrict__ hdr, const uint32_t* __restrict__ vis_list, const uint32_t* __restrict__ offsets,
               const float4* __restrict__ ws, uint32_t ws_slots, int C, int c0, int accumulate, float* __restrict__ dL_dfeatures)
{
    const uint32_t n = hdr->num_compact;
    if (n == 0) return;
    if (hdr->overflow != 0u) return;                                  // async mode: an overflowed view contributes nothing
    const uint32_t n_slots = hdr->num_sorted;                         // slots beyond were never built
    if (n_slots > ws_slots) {
        // the caller's workspace does not hold the view (exact mode: `slots` below the forward's instance count): lr_check
        // reports it as an incomplete backward; no row outside the workspace is read or was written
        if (blockIdx.x == 0 && threadIdx.x == 0) hdr->bwd_uncovered = 1u;
    }
    const uint32_t lim = min(n_slots, ws_slots);
    const int lane = threadIdx.x & 63;
    for (uint32_t t0 = blockIdx.x * FR_THREADS; t0 < n; t0 += gridDim.x * FR_THREADS) {
        const uint32_t t = t0 + threadIdx.x;
        const bool live = t < n;
        const uint32_t idx = live ? vis_list[t] : 0u;
        const uint32_t off = live ? offsets[t] : 0u;
        const uint32_t tt = live ? ((t + 1 < n) ? offsets[t + 1] : hdr->num_instances) - off : 0u;
        float4 acc[K / 4];
#pragma unroll
        for (int q = 0; q < K / 4; q++) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tt <= FR_SERIAL_MAX && off < lim) {
            const uint32_t cnt = min(tt, lim - off);
            const float4* r = ws + (size_t)off * (K / 4);
            for (uint32_t j = 0; j < cnt; j++) {
#pragma unroll
                for (int q = 0; q < K / 4; q++) {
                    const float4 v = r[(size_t)j * (K / 4) + q];
                    acc[q].x += v.x; acc[q].y += v.y; acc[q].z += v.z; acc[q].w += v.w;
                }
            }
        }
        uint64_t big = __ballot(tt > FR_SERIAL_MAX);
        while (big) {
            const int src = __ffsll((long long)big) - 1;
            big &= big - 1;
            const uint32_t b_tt = __shfl(tt, src), b_off = __shfl(off, src);
            float4 p[K / 4];
#pragma unroll
            for (int q = 0; q < K / 4; q++) p[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (uint32_t j = lane; j < b_tt; j += 64) {
                if (b_off + j >= lim) break;
                const float4* r = ws + (size_t)(b_off + j) * (K / 4);
#pragma unroll
                for (int q = 0; q < K / 4; q++) {
                    const float4 v = r[q];
                    p[q].x += v.x; p[q].y += v.y; p[q].z += v.z; p[q].w += v.w;
                }
            }
#pragma unroll
            for (int q = 0; q < K / 4; q++) {
                p[q].x = ftr_wave_sum(p[q].x); p[q].y = ftr_wave_sum(p[q].y);
                p[q].z = ftr_wave_sum(p[q].z); p[q].w = ftr_wave_sum(p[q].w);
            }
            if (lane == src) {
#pragma unroll
                for (int q = 0; q < K / 4; q++) acc[q] = p[q];
            }
        }
        if (live) {
            float* o = dL_dfeatures + (size_t)idx * C + c0;
            const int left = C - c0;
#pragma unroll
            for (int q = 0; q < K / 4; q++) {
                const float v[4] = { acc[q].x, acc[q].y, acc[q].z, acc[q].w };
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (4 * q + k < left) o[4 * q + k] = accumulate ? o[4 * q + k] + v[k] : v[k];
            }
        }
    }
}

inline bool features_vec(const float* features, int C) { return (C & 3) == 0 && (reinterpret_cast<uintptr_t>(features) & 15u) == 0; }

}  // namespace

int features_chunk() { return FTR_K; }

size_t features_workspace_bytes(long long slots) { return align_up((size_t)(slots > 0 ? slots : 1) * FTR_K * sizeof(float)); }

void launch_render_features(int W, int H, int P, const GeomView& g, const ImgView& im, const char* bin_base, const float* features,
                            int C, float* out_features, hipStream_t s)
{
    const TileGrid t = tile_grid(W, H);
    if (t.num_tiles <= 0) return;
    if (P <= 0) {                                                     // the forward of an empty cloud wrote no header and no list
        const long long n = (long long)C * W * H;
        hipLaunchKernelGGL(k_features_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, out_features);
        return;
    }
    const int vec = features_vec(features, C) ? 1 : 0;
    dispatch_strict([&](auto st) {
        for (int c0 = 0; c0 < C; c0 += FTR_K)
            hipLaunchKernelGGL((k_render_features<st.value, FTR_K>), dim3(t.grid), dim3(WALK_THREADS), 0, s, W, H, t.gx, t.num_tiles,
                               t.tile_map, im.ranges, bin_base, g.rec, g.header, features, C, c0, vec, out_features);
    });
}

void launch_features_bwd(int W, int H, int P, const GeomView& g, const ImgView& im, char* bin_base, const float* dL_dout_features,
                         const float* out_features, const float* features, int C, char* workspace, size_t workspace_bytes,
                         bool accumulate, float* dL_dfeatures, hipStream_t s)
{
    const TileGrid t = tile_grid(W, H);
    if (P <= 0 || t.num_tiles <= 0) return;
    const int vec = features_vec(features, C) ? 1 : 0;
    const size_t rows = workspace_bytes / (FTR_K * sizeof(float));
    const uint32_t ws_slots = rows > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rows;
    float4* ws = reinterpret_cast<float4*>(workspace);
    const unsigned row_blocks = (unsigned)min((P + FR_THREADS - 1) / FR_THREADS, 2048);
    dispatch_strict([&](auto st) {
        for (int c0 = 0; c0 < C; c0 += FTR_K) {
            hipLaunchKernelGGL((k_features_bwd<st.value, FTR_K>), dim3(t.grid), dim3(WALK_THREADS), 0, s, W, H, t.gx, t.num_tiles,
                               t.tile_map, im.ranges, bin_base, g.rec, g.header, dL_dout_features, out_features, features, C, c0,
                               vec, ws, ws_slots);
            hipLaunchKernelGGL((k_feature_rows<FTR_K>), dim3(row_blocks), dim3(FR_THREADS), 0, s, g.header, g.vis_list, g.offsets,
                               ws, ws_slots, C, c0, accumulate ? 1 : 0, dL_dfeatures);
        }
    });
}

}  // namespace lr
