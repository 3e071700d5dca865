// render_median.hip -- median depth and per-pixel Gaussian ids of a finished forward, and the gradient of the median depth, for gfx950.
//
// Definition.  For one pixel, walk its tile's list front to back exactly as the blend forward does (render_fwd.hip), T = 1 at
// the start:
//     power > 0                                  -> skip
//     alpha = min(0.99, opacity exp(power));  alpha < 1/255 -> skip
//     test_T = T (1 - alpha);  test_T < 1e-4     -> stop, not blended
//     otherwise blend: T = test_T
// The MEDIAN Gaussian of the pixel is the first blended Gaussian with test_T < 0.5: the layer at which the transmittance first
// falls below one half.
//     median_depth [1,H,W] float32 : that Gaussian's view-space z (GaussRec::depth, the per-Gaussian value the expected depth
//                                    blends); 0 where T never falls below 0.5 -- the depth output's own "0 = no surface"
//     median_ids   [H,W]   int32   : its row in the caller's P rows; -1 where there is none
// The two thresholds never interact: alpha <= 0.99, so a pixel still at T >= 0.5 has test_T >= 0.5 (1 - 0.99) > 1e-4 -- the
// 1e-4 stop cannot trigger in front of the median, and the walk below does not test it.
// The values hold under strict parity, anti-aliasing, the 3D filter, raw and activated parameters and both forward shapes: all of
// that already sits in the GaussRec records and the tile lists, and the walk (tile_walk.h) evaluates alpha with the arithmetic of
// the forward that produced the state, on the same staged coefficients, in the same order.  Its T sequence is the forward's bit
// for bit up to the median.
//
// A pass of its own (as lr_render_alpha): the blend-forward kernels stay as they are.  It stops at T < 0.5, far earlier than the
// blend's T < 1e-4, and carries no colour.
//
// Forward, k_render_median: the quadrant walk of tile_walk.h (shape, staging, cull and alpha arithmetic are there), 256 list
// entries per round; the value it keeps per staged entry is the view depth, and the Gaussian id is staged beside it (44 bytes per
// entry in all).  A quadrant stops when every pixel of it has its median or the list ends; a view whose header says `overflow`
// writes 0 / -1 everywhere.
//
// Gradient.  The selection of the median Gaussian is a constant (as the sort order is everywhere else), so
//     d median_depth[p] / d z_g = 1   for g = median_ids[p], nothing else:
// it reaches dL/dmean3D[g] (raw mode: dL/dxyz) through z = view[2] x + view[6] y + view[10] z + view[14]; nothing flows to
// opacity, covariance or colour.  A weaker signal than the expected depth's gradient (which also moves opacities and shapes),
// enough to put a depth loss on the median depth.
//
// Backward, k_median_bwd / k_median_bwd_wide: a GATHER, no global float atomics, bit-repeatable.  Per emitting Gaussian (vis_list)
// the pixels of a box that holds every pixel it can be the median of (med_box: its tile rectangle cut down to the bounding box of
// its alpha >= 1/255 ellipse) are read in a fixed order and dL is summed where ids == g: lane-strided partial sums, one
// fixed-order wave reduction, one store (or add) of s (view[2], view[6], view[10]).  A Gaussian's sum depends on nothing but its
// own box -- not on the grid, not on which wave takes it.  Skew: a few Gaussians cover thousands of tiles.  Boxes of up to
// MB_WAVE_PIX pixels are summed by one wave; larger ones by a whole 1024-thread workgroup of the second kernel: wave w takes the
// 64-pixel chunks w, w + 16, ... and the 16 partial sums are added in wave order.
#include "common.h"
#include "tile_walk.h"

namespace lr {

namespace {

constexpr int MED_BATCH = 256;          // staged list entries per round (11 KB of LDS)

template <bool STRICT>
__global__ void __launch_bounds__(WALK_THREADS)
k_render_median(int W, int H, int gx, int num_tiles, int tile_map, const uint2* __restrict__ ranges,
                const char* __restrict__ bin_base, const GaussRec* __restrict__ rec, const GeomHeader* __restrict__ hdr,
                float* __restrict__ out_depth, int* __restrict__ out_ids)
{
    __shared__ float4 s_q0[MED_BATCH];      // WalkPlanes; the value kept in s_q1[].z: view depth
    __shared__ float4 s_q1[MED_BATCH];
    __shared__ float2 s_q3[MED_BATCH];
    __shared__ uint32_t s_id[MED_BATCH];
    __shared__ int s_wdone[WALK_WAVES];

    const int tile = blend_tile(tile_map, num_tiles);
    if (tile < 0) return;
    const QuadLane q = quad_lane(tile, gx, W, H);
    const TileList tl = tile_list(hdr, ranges, bin_base, tile);     // overflowed: empty, no median anywhere

    float T = 1.0f, med_depth = 0.0f;
    int med_id = -1;
    uint64_t done = __builtin_amdgcn_ballot_w64(!q.inside);           // pixels that have their median (or lie outside the image)

    tile_walk<STRICT, MED_BATCH>(
        q, tl, rec, WalkPlanes{s_q0, s_q1, s_q3, s_wdone}, done,
        [&](int slot, uint32_t id, float z) { s_id[slot] = id; return z; },
        [&](int, float, float alpha, uint64_t use) {
            const float test_T = T * (1.0f - alpha);
            // the forward's T < 1e-4 stop cannot trigger while T >= 0.5 (header comment)
            const uint64_t found = use & __builtin_amdgcn_ballot_w64(test_T < 0.5f);
            T = __builtin_amdgcn_inverse_ballot_w64(use) ? test_T : T;
            return found;
        },
        [&](int j, float z, uint64_t found) {
            if (__builtin_amdgcn_inverse_ballot_w64(found)) { med_depth = z; med_id = (int)s_id[j]; }
        });

    if (q.inside) {
        const size_t pix = (size_t)q.py * W + q.px;
        out_depth[pix] = med_depth;
        if (out_ids != nullptr) out_ids[pix] = med_id;
    }
}

// a view without a list to read (P = 0): 0 / -1 everywhere
__global__ void __launch_bounds__(256) k_median_fill(long long n, float* __restrict__ out_depth, int* __restrict__ out_ids)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        out_depth[i] = 0.0f;
        if (out_ids != nullptr) out_ids[i] = -1;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
constexpr int MB_WAVE_PIX = 64 * 64;        // boxes of up to 4096 pixels: one wave, at most 64 pixels per lane
constexpr int MB_WIDE_THREADS = 1024;
constexpr int MB_WIDE_WAVES = MB_WIDE_THREADS / 64;
constexpr int MB_UNROLL = 8;                // pixels per lane and trip of the gather
constexpr int MB_ROUND = 16;              // list entries per round of the one-wave kernel
constexpr int MB_MAX_GROUPS = 256 * 4 * 8;  // its persistent workgroups: CUs x SIMDs x resident waves

__device__ __forceinline__ float med_wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);     // a fixed tree: every lane ends with the same bits
    return v;
}

// Pixel box [bx, bx + bw) x [by, by + bh) that holds every pixel Gaussian g can be the median of; returns its pixel count.
// Two bounds, intersected: the tile rectangle (every tile that lists g lies inside), clipped to the image, and the bounding
// box of the ellipse 0.5 (a dx^2 + c dy^2) + b dx dy <= qmax -- a pixel that blended g reached alpha >= 1/255, i.e.
// q <= log(255 opacity), and qmax is that plus CULL_MARGIN (the bound the forward's own cull relies on): half-widths
// sqrt(2 qmax c / det) and sqrt(2 qmax a / det), one more pixel for their rounding.  For the pixel-sized splats of a real scene
// this is tens of pixels where the rectangle has hundreds.  Not a proper ellipse (or NaN): the rectangle alone.
__device__ __forceinline__ uint32_t med_box(const GaussRec* __restrict__ rec, const int* __restrict__ radii, uint32_t g,
                                             int W, int H, int gx, int gy, int& bx, int& by, int& bw)
{
    const float4* r4 = reinterpret_cast<const float4*>(rec + g);
    const float4 a = r4[0];                                             // x, y, conic a, conic b
    const float cc = r4[1].x, qmax = r4[2].z;
    int minx, miny, maxx, maxy;
    tile_rect(a.x, a.y, radii[g], gx, gy, minx, miny, maxx, maxy);
    float x_lo = (float)(minx * TILE_X), x_hi = (float)min(W, maxx * TILE_X);       // [lo, hi)
    float y_lo = (float)(miny * TILE_Y), y_hi = (float)min(H, maxy * TILE_Y);
    bx = 0; by = 0; bw = 1;
    if (!(qmax > 0.0f)) return 0u;                                      // cannot reach 1/255 anywhere
    const float det = a.z * cc - a.w * a.w;
    if (det > 0.0f && a.z > 0.0f && cc > 0.0f) {
        const float k = 2.0f * qmax / det;
        const float hx = sqrtf(k * cc) + 1.0f, hy = sqrtf(k * a.z) + 1.0f;
        x_lo = fmaxf(x_lo, ceilf(a.x - hx)); x_hi = fminf(x_hi, floorf(a.x + hx) + 1.0f);      // (fmaxf / fminf drop a NaN)
        y_lo = fmaxf(y_lo, ceilf(a.y - hy)); y_hi = fminf(y_hi, floorf(a.y + hy) + 1.0f);
    }
    if (!(x_hi > x_lo) || !(y_hi > y_lo)) return 0u;
    bx = (int)x_lo; by = (int)y_lo;                                     // all four lie in [0, W] / [0, H]
    bw = (int)x_hi - bx;
    return (uint32_t)bw * (uint32_t)((int)y_hi - by);                   // (the entry point holds W H below 2^31)
}

// this lane's share of the box: pixels first, first + stride, ... below n, in that order
__device__ __forceinline__ float med_gather(const float* __restrict__ dL, const int* __restrict__ ids, int g, int W,
                                            int bx, int by, int bw, uint32_t first, uint32_t stride, uint32_t n)
{
    // MB_UNROLL pixels per trip: their ids loads are in flight together, then the dL loads of the matches; added in pixel order
    float s = 0.0f;
    for (uint32_t i0 = first; i0 < n; i0 += MB_UNROLL * stride) {
        int idv[MB_UNROLL];
        uint32_t pixv[MB_UNROLL];
#pragma unroll
        for (int u = 0; u < MB_UNROLL; u++) {
            const uint32_t i = i0 + (uint32_t)u * stride;
            idv[u] = -2; pixv[u] = 0u;                                  // (-2: no pixel; a Gaussian's id is never negative)
            if (i < n) {
                const uint32_t ry = i / (uint32_t)bw, rx = i - ry * (uint32_t)bw;
                pixv[u] = (uint32_t)(by + (int)ry) * (uint32_t)W + (uint32_t)(bx + (int)rx);
                idv[u] = ids[pixv[u]];
            }
        }
#pragma unroll
        for (int u = 0; u < MB_UNROLL; u++)
            if (idv[u] == g) s += dL[pixv[u]];
    }
    return s;
}

__device__ __forceinline__ void med_store(float* __restrict__ dL_dmean3D, uint32_t g, float s, const float* __restrict__ view,
                                          int accumulate)
{
    float* o = dL_dmean3D + 3 * (size_t)g;
    const float gx_ = s * view[2], gy_ = s * view[6], gz_ = s * view[10];
    if (accumulate) { o[0] += gx_; o[1] += gy_; o[2] += gz_; }
    else { o[0] = gx_; o[1] = gy_; o[2] = gz_; }
}

// One wave per emitting Gaussian; rounds of MB_ROUND list entries dealt round-robin over persistent single-wave workgroups.  The
// kernel is a chain of dependent loads (list -> record, radius -> ids -> dL): the first two links are taken once per round,
// lane j for entry j, and what is left per Gaussian is the gather itself; many short rounds keep many waves in flight.
__global__ void __launch_bounds__(64)
k_median_bwd(int W, int H, int gx, int gy, const GeomHeader* __restrict__ hdr, const uint32_t* __restrict__ vis_list,
             const GaussRec* __restrict__ rec, const int* __restrict__ radii, const float* __restrict__ dL, const int* __restrict__ ids,
             const float* __restrict__ view, float* __restrict__ dL_dmean3D, int accumulate)
{
    if (hdr->overflow != 0u) return;
    const uint32_t n_vis = hdr->num_compact;
    const int l = threadIdx.x;
    for (uint32_t k0 = blockIdx.x * MB_ROUND; k0 < n_vis; k0 += gridDim.x * MB_ROUND) {
        uint32_t g = 0u, n = 0u;
        int bx = 0, by = 0, bw = 1;
        if (l < MB_ROUND && k0 + (uint32_t)l < n_vis) {
            g = vis_list[k0 + l];
            n = med_box(rec, radii, g, W, H, gx, gy, bx, by, bw);
        }
        // Boxes of up to 64 pixels (the bulk: pixel-sized splats) are one pixel per lane.  Their ids loads are issued for the
        // whole round before any is waited for, then their dL loads: two latencies per round instead of two per Gaussian.  The
        // value a lane ends with is what med_gather's stride-64 walk gives it (at most one pixel), so the sums are the same bits.
        int idv[MB_ROUND];
        uint32_t pixv[MB_ROUND];
        float v[MB_ROUND];
#pragma unroll
        for (int j = 0; j < MB_ROUND; j++) {
            const uint32_t nj = (uint32_t)__builtin_amdgcn_readlane((int)n, j);
            idv[j] = -2; pixv[j] = 0u;                                 // (-2: no pixel; a Gaussian's id is never negative)
            if (nj != 0u && nj <= 64u && (uint32_t)l < nj) {
                const uint32_t bwj = (uint32_t)__builtin_amdgcn_readlane(bw, j);
                const uint32_t ry = (uint32_t)l / bwj, rx = (uint32_t)l - ry * bwj;
                pixv[j] = (uint32_t)(__builtin_amdgcn_readlane(by, j) + (int)ry) * (uint32_t)W + (uint32_t)(__builtin_amdgcn_readlane(bx, j) + (int)rx);
                idv[j] = ids[pixv[j]];
            }
        }
#pragma unroll
        for (int j = 0; j < MB_ROUND; j++)
            v[j] = idv[j] == __builtin_amdgcn_readlane((int)g, j) ? dL[pixv[j]] : 0.0f;
        float mine = 0.0f;                                             // lane j: the sum of entry j
#pragma unroll
        for (int j = 0; j < MB_ROUND; j++) {
            const uint32_t nj = (uint32_t)__builtin_amdgcn_readlane((int)n, j);
            if (nj == 0u || nj > (uint32_t)MB_WAVE_PIX) continue;      // nothing to add (the row is zero-filled); k_median_bwd_wide's
            float s = v[j];
            if (nj > 64u)
                s = med_gather(dL, ids, __builtin_amdgcn_readlane((int)g, j), W, __builtin_amdgcn_readlane(bx, j),
                               __builtin_amdgcn_readlane(by, j), __builtin_amdgcn_readlane(bw, j), l, 64, nj);
            s = med_wave_sum(s);
            if (l == j) mine = s;
        }
        // the round's rows, lane j its own: one read-modify-write latency per round
        if (l < MB_ROUND && n != 0u && n <= (uint32_t)MB_WAVE_PIX) med_store(dL_dmean3D, g, mine, view, accumulate);
    }
}

// the boxes beyond MB_WAVE_PIX pixels: a workgroup scans 1024 list entries at a time and sums each wide one with all 16 waves
__global__ void __launch_bounds__(MB_WIDE_THREADS)
k_median_bwd_wide(int W, int H, int gx, int gy, const GeomHeader* __restrict__ hdr, const uint32_t* __restrict__ vis_list,
                  const GaussRec* __restrict__ rec, const int* __restrict__ radii, const float* __restrict__ dL,
                  const int* __restrict__ ids, const float* __restrict__ view, float* __restrict__ dL_dmean3D, int accumulate)
{
    __shared__ uint32_t s_wide[MB_WIDE_THREADS];
    __shared__ int s_n;
    __shared__ float s_part[MB_WIDE_WAVES];
    if (hdr->overflow != 0u) return;
    const uint32_t n_vis = hdr->num_compact;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    for (uint32_t k0 = blockIdx.x * MB_WIDE_THREADS; k0 < n_vis; k0 += gridDim.x * MB_WIDE_THREADS) {
        if (tid == 0) s_n = 0;
        lds_barrier();
        const uint32_t k = k0 + tid;
        if (k < n_vis) {
            const uint32_t g = vis_list[k];
            int bx, by, bw;
            if (med_box(rec, radii, g, W, H, gx, gy, bx, by, bw) > (uint32_t)MB_WAVE_PIX) s_wide[atomicAdd(&s_n, 1)] = g;   // (LDS, integers)
        }
        lds_barrier();
        const int n_wide = s_n;
        for (int i = 0; i < n_wide; i++) {                             // each one's sum is its own: their order does not matter
            const uint32_t g = s_wide[i];
            int bx, by, bw;
            const uint32_t n = med_box(rec, radii, g, W, H, gx, gy, bx, by, bw);
            const float s = med_wave_sum(med_gather(dL, ids, (int)g, W, bx, by, bw, tid, MB_WIDE_THREADS, n));
            if (l == 0) s_part[w] = s;
            lds_barrier();
            if (tid == 0) {
                float t = 0.0f;
#pragma unroll
                for (int j = 0; j < MB_WIDE_WAVES; j++) t += s_part[j];
                med_store(dL_dmean3D, g, t, view, accumulate);
            }
            lds_barrier();
        }
    }
}

}  // namespace

void launch_render_median(int W, int H, int P, const GeomView& g, const ImgView& im, const char* bin_base, float* out_depth,
                          int* out_ids, hipStream_t s)
{
    const TileGrid t = tile_grid(W, H);
    if (t.num_tiles <= 0) return;
    if (P <= 0) {                                                     // the forward of an empty cloud wrote no header and no list
        const long long n = (long long)W * H;
        hipLaunchKernelGGL(k_median_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, out_depth, out_ids);
        return;
    }
    dispatch_strict([&](auto st) {
        hipLaunchKernelGGL((k_render_median<st.value>), dim3(t.grid), dim3(WALK_THREADS), 0, s, W, H, t.gx, t.num_tiles, t.tile_map,
                           im.ranges, bin_base, g.rec, g.header, out_depth, out_ids);
    });
}

void launch_median_bwd(int W, int H, int P, const GeomView& g, const int* radii, const int* ids, const float* dL_dmedian,
                       const float* view, float* dL_dmean3D, bool accumulate, hipStream_t s)
{
    if (P <= 0 || W <= 0 || H <= 0) return;
    const int gx = (W + TILE_X - 1) / TILE_X, gy = (H + TILE_Y - 1) / TILE_Y;
    const int groups = min((P + MB_ROUND - 1) / MB_ROUND, MB_MAX_GROUPS);
    hipLaunchKernelGGL(k_median_bwd, dim3(groups), dim3(64), 0, s, W, H, gx, gy, g.header, g.vis_list, g.rec, radii, dL_dmedian, ids,
                       view, dL_dmean3D, accumulate ? 1 : 0);
    // only a footprint beyond MB_WAVE_PIX pixels is left to the second kernel: an image that small has none
    if ((long long)W * H > (uint32_t)MB_WAVE_PIX) {
        const int wide_groups = min((P + MB_WIDE_THREADS - 1) / MB_WIDE_THREADS, 256);
        hipLaunchKernelGGL(k_median_bwd_wide, dim3(wide_groups), dim3(MB_WIDE_THREADS), 0, s, W, H, gx, gy, g.header, g.vis_list, g.rec,
                           radii, dL_dmedian, ids, view, dL_dmean3D, accumulate ? 1 : 0);
    }
}

}  // namespace lr
