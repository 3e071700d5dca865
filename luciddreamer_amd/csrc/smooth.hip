// smooth.hip -- edge-aware smoothness of a rendered map (depth, inverse depth, normals) for gfx950 (include/lucid_raster.h,
// lr_smooth_args).
//
// The definition is the header's, operation by operation (this file is compiled with -ffp-contract=off; hipcc's float division
// is correctly rounded): a numpy restatement differs by the device's expf alone.
//   k_smooth_fwd<ORDER>  : one pixel per lane and row, FWD_ROWS rows of 64 pixels per workgroup.  A pixel OWNS the terms that
//                          start at it (order 1: the pairs to its right and below) or are centred on it (order 2: the two
//                          triples), so every term is formed exactly once; {sum, count} per workgroup, double, fixed order.
//   k_smooth_final       : one workgroup sums the partials in a fixed order -> {loss, count}.
//   k_smooth_bwd<ORDER>  : the gather: a pixel walks the terms it belongs to (4 at order 1, 6 at order 2) in the header's order
//                          and recomputes each one's weight and signs from the inputs.  No atomics, no workspace.
// A wave covers 64 consecutive pixels of one row, so every global load and store is coalesced; the neighbour reads (the same
// rows shifted by one or two pixels, the rows above and below) are served by the vector L1 / L2 and are not staged in LDS:
// DESIGN.md 4b-SMO has the bytes and the times of this shape and of an LDS-staged rival.
#include "common.h"
#include "wave_reduce.h"
#include <cmath>

namespace lr {

namespace {

constexpr int SB_X = 64;                   // a wave is one row segment
constexpr int SB_Y = 4;
constexpr int NTHREADS = SB_X * SB_Y;      // 256
constexpr int FWD_ROWS = 16;               // rows per workgroup of the forward: 4 pixels per thread, a quarter of the partials
constexpr int MAX_C = 4, MAX_G = 3;

struct Smooth {
    int H, W, C, G;                        // G = 0: no guide
    const float* map;
    const float* guide;
    const float* mask;
    int inverse, positive_only;
    float gamma;
};

// One pixel: is it valid, its values u (1 / map in inverse space) and its guide colours.  Nothing is loaded for coordinates
// outside the image, so every address is inside it.
struct Pix {
    bool valid;
    float u[MAX_C];
    float g[MAX_G];
};

__device__ __forceinline__ Pix load_pix(const Smooth& s, int x, int y)
{
    Pix p;
    p.valid = false;
#pragma unroll
    for (int c = 0; c < MAX_C; c++) p.u[c] = 0.f;
#pragma unroll
    for (int c = 0; c < MAX_G; c++) p.g[c] = 0.f;
    if (x < 0 || y < 0 || x >= s.W || y >= s.H) return p;
    const size_t n = (size_t)s.H * (size_t)s.W, i = (size_t)y * (size_t)s.W + (size_t)x;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < MAX_C; c++)
        if (c < s.C) {
            p.u[c] = s.map[i + (size_t)c * n];
            ok = ok && fabsf(p.u[c]) < INFINITY;                 // NaN fails
        }
    if (s.positive_only) ok = ok && p.u[0] > 0.f;
    if (s.mask != nullptr) ok = ok && s.mask[i] > 0.f;
    if (s.inverse) {
        p.u[0] = 1.0f / p.u[0];
        ok = ok && p.u[0] < INFINITY;                           // a subnormal depth whose reciprocal overflows
    }
#pragma unroll
    for (int c = 0; c < MAX_G; c++)
        if (c < s.G) p.g[c] = s.guide[i + (size_t)c * n];
    p.valid = ok;
    return p;
}

__device__ __forceinline__ float nan_max(float l, float r) { return (l > r || l != l) ? l : r; }     // a NaN on either side stays

// the mean over the guide's channels of d[]
__device__ __forceinline__ float guide_mean(const Smooth& s, const float* d)
{
    return s.G == 3 ? ((d[0] + d[1]) + d[2]) / 3.0f : d[0];
}

// Does the term count (its pixels are valid and its guide difference is finite)?  Then w is its weight.
__device__ __forceinline__ bool weight_of(const Smooth& s, float a, float& w)
{
    if (!(a >= 0.f && a < INFINITY)) return false;          // NaN, or an infinite guide value on one side: gamma a = 0 inf at gamma = 0
    w = s.G > 0 ? expf(-(s.gamma * a)) : 1.0f;
    return true;
}

// order 1: the pair (p, q), q the pixel to the right of or below p
__device__ __forceinline__ bool pair_weight(const Smooth& s, const Pix& p, const Pix& q, float& w)
{
    if (!(p.valid && q.valid)) return false;
    float d[MAX_G];
#pragma unroll
    for (int c = 0; c < MAX_G; c++) d[c] = fabsf(p.g[c] - q.g[c]);
    return weight_of(s, guide_mean(s, d), w);
}
__device__ __forceinline__ double pair_delta(const Pix& p, const Pix& q, int c) { return (double)q.u[c] - (double)p.u[c]; }

// order 2: the triple (m, p, q) centred on p
__device__ __forceinline__ bool triple_weight(const Smooth& s, const Pix& m, const Pix& p, const Pix& q, float& w)
{
    if (!(m.valid && p.valid && q.valid)) return false;
    float d[MAX_G];
#pragma unroll
    for (int c = 0; c < MAX_G; c++) d[c] = nan_max(fabsf(p.g[c] - m.g[c]), fabsf(q.g[c] - p.g[c]));
    return weight_of(s, guide_mean(s, d), w);
}
__device__ __forceinline__ double triple_delta(const Pix& m, const Pix& p, const Pix& q, int c)
{
    return ((double)m.u[c] - 2.0 * (double)p.u[c]) + (double)q.u[c];
}

// ---- forward ----
__device__ __forceinline__ void count_pair(const Smooth& s, const Pix& p, const Pix& q, double& v, int& counted)
{
    float w;
    if (!pair_weight(s, p, q, w)) return;
    double t = 0.0;
#pragma unroll
    for (int c = 0; c < MAX_C; c++)
        if (c < s.C) t += fabs(pair_delta(p, q, c));
    v += (double)w * t;
    counted += 1;
}

__device__ __forceinline__ void count_triple(const Smooth& s, const Pix& m, const Pix& p, const Pix& q, double& v, int& counted)
{
    float w;
    if (!triple_weight(s, m, p, q, w)) return;
    double t = 0.0;
#pragma unroll
    for (int c = 0; c < MAX_C; c++)
        if (c < s.C) t += fabs(triple_delta(m, p, q, c));
    v += (double)w * t;
    counted += 1;
}

template <int ORDER>
__global__ void __launch_bounds__(NTHREADS)
k_smooth_fwd(Smooth s, int blocks_x, double2* __restrict__ partials)
{
    __shared__ double s_sum[NTHREADS / 64];
    __shared__ int s_cnt[NTHREADS / 64];
    const int bx = (int)(blockIdx.x % (unsigned)blocks_x), by = (int)(blockIdx.x / (unsigned)blocks_x);
    const int x = bx * SB_X + (int)(threadIdx.x & (SB_X - 1));
    double v = 0.0;
    int counted = 0;
#pragma unroll
    for (int i = 0; i < FWD_ROWS / SB_Y; i++) {          // rows ty, ty + 4, ...: summed in this order, horizontal term first
        const int y = by * FWD_ROWS + i * SB_Y + (int)(threadIdx.x / SB_X);
        if (x >= s.W || y >= s.H) continue;
        const Pix p = load_pix(s, x, y);
        if (!p.valid) continue;
        if (ORDER == 1) {
            count_pair(s, p, load_pix(s, x + 1, y), v, counted);
            count_pair(s, p, load_pix(s, x, y + 1), v, counted);
        } else {
            count_triple(s, load_pix(s, x - 1, y), p, load_pix(s, x + 1, y), v, counted);
            count_triple(s, load_pix(s, x, y - 1), p, load_pix(s, x, y + 1), v, counted);
        }
    }
    v = wave_sum(v);
    counted = wave_sum(counted);
    const int wv = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_sum[wv] = v; s_cnt[wv] = counted; }
    lds_barrier();
    if (threadIdx.x == 0)
        partials[blockIdx.x] = make_double2((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]),
                                            (double)((s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3])));
}

__global__ void __launch_bounds__(NTHREADS)
k_smooth_final(int n_blocks, double n_elems, float weight, const double2* __restrict__ partials, float* __restrict__ out)
{
    __shared__ double s_a[NTHREADS], s_b[NTHREADS];
    double a = 0.0, b = 0.0;
    for (int i = (int)threadIdx.x; i < n_blocks; i += NTHREADS) { const double2 p = partials[i]; a += p.x; b += p.y; }
    s_a[threadIdx.x] = a; s_b[threadIdx.x] = b;
    lds_barrier();
    for (int off = NTHREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { s_a[threadIdx.x] += s_a[threadIdx.x + off]; s_b[threadIdx.x] += s_b[threadIdx.x + off]; }
        lds_barrier();
    }
    if (threadIdx.x == 0) {
        out[0] = weight * (float)(s_a[0] / n_elems);
        out[1] = (float)s_b[0];
    }
}

// ---- backward ----
__device__ __forceinline__ float sign_of(double d) { return (float)((d > 0.0) - (d < 0.0)); }

// g[c] += (coef w) sign(delta_c) of the pair (p, q): coef = -1 for p, +1 for q.  Both products are exact (coef and the sign
// are 0, +-1 or -2), and without an edge w = 1: terms that cancel as integers leave an exact zero.
__device__ __forceinline__ void gather_pair(const Smooth& s, const Pix& p, const Pix& q, float coef, float* g)
{
    float w;
    if (!pair_weight(s, p, q, w)) return;
    const float cw = coef * w;
#pragma unroll
    for (int c = 0; c < MAX_C; c++)
        if (c < s.C) g[c] += cw * sign_of(pair_delta(p, q, c));
}

// ... of the triple (m, p, q): coef = 1 for m and q, -2 for p
__device__ __forceinline__ void gather_triple(const Smooth& s, const Pix& m, const Pix& p, const Pix& q, float coef, float* g)
{
    float w;
    if (!triple_weight(s, m, p, q, w)) return;
    const float cw = coef * w;
#pragma unroll
    for (int c = 0; c < MAX_C; c++)
        if (c < s.C) g[c] += cw * sign_of(triple_delta(m, p, q, c));
}

template <int ORDER>
__global__ void __launch_bounds__(NTHREADS)
k_smooth_bwd(Smooth s, int blocks_x, float weight, const float* __restrict__ upstream, float* __restrict__ grad)
{
    const int bx = (int)(blockIdx.x % (unsigned)blocks_x), by = (int)(blockIdx.x / (unsigned)blocks_x);
    const int x = bx * SB_X + (int)(threadIdx.x & (SB_X - 1));
    const int y = by * SB_Y + (int)(threadIdx.x / SB_X);
    if (x >= s.W || y >= s.H) return;
    const float up = upstream != nullptr ? upstream[0] : 1.0f;
    const float k = (up * weight) / (float)(s.H * s.W);
    float g[MAX_C] = { 0.f, 0.f, 0.f, 0.f };
    const Pix p = load_pix(s, x, y);
    if (p.valid) {
        if (ORDER == 1) {
            gather_pair(s, load_pix(s, x - 1, y), p, 1.f, g);                 // horizontal, left to right
            gather_pair(s, p, load_pix(s, x + 1, y), -1.f, g);
            gather_pair(s, load_pix(s, x, y - 1), p, 1.f, g);                 // vertical, top to bottom
            gather_pair(s, p, load_pix(s, x, y + 1), -1.f, g);
        } else {
            {
                const Pix l = load_pix(s, x - 1, y), r = load_pix(s, x + 1, y);
                gather_triple(s, load_pix(s, x - 2, y), l, p, 1.f, g);        // centred on x - 1, x, x + 1
                gather_triple(s, l, p, r, -2.f, g);
                gather_triple(s, p, r, load_pix(s, x + 2, y), 1.f, g);
            }
            {
                const Pix t = load_pix(s, x, y - 1), b = load_pix(s, x, y + 1);
                gather_triple(s, load_pix(s, x, y - 2), t, p, 1.f, g);        // centred on y - 1, y, y + 1
                gather_triple(s, t, p, b, -2.f, g);
                gather_triple(s, p, b, load_pix(s, x, y + 2), 1.f, g);
            }
        }
#pragma unroll
        for (int c = 0; c < MAX_C; c++) g[c] = k * g[c];
        if (s.inverse) g[0] = -(g[0] * p.u[0]) * p.u[0];
    }
    const size_t n = (size_t)s.H * (size_t)s.W, i = (size_t)y * (size_t)s.W + (size_t)x;
#pragma unroll
    for (int c = 0; c < MAX_C; c++)
        if (c < s.C) grad[i + (size_t)c * n] = g[c];
}

Smooth smooth_of(const lr_smooth_args& a)
{
    Smooth s;
    s.H = a.height;
    s.W = a.width;
    s.C = a.channels;
    s.G = a.guide != nullptr ? a.guide_channels : 0;
    s.map = a.map;
    s.guide = a.guide;
    s.mask = a.mask;
    s.inverse = a.space == LR_SMOOTH_INVERSE ? 1 : 0;
    s.positive_only = a.positive_only;
    s.gamma = a.gamma;
    return s;
}

int blocks_x_of(int W) { return (W + SB_X - 1) / SB_X; }
int blocks_of(int H, int W, int rows) { return blocks_x_of(W) * ((H + rows - 1) / rows); }     // <= H*W < 2^31

}  // namespace

size_t smooth_workspace_bytes(int H, int W) { return align_up((size_t)blocks_of(H, W, FWD_ROWS) * sizeof(double2)); }

void launch_smooth_forward(const lr_smooth_args& a, hipStream_t s)
{
    const int blocks = blocks_of(a.height, a.width, FWD_ROWS), bx = blocks_x_of(a.width);
    double2* partials = static_cast<double2*>(a.workspace);
    if (a.order == 1)
        hipLaunchKernelGGL(k_smooth_fwd<1>, dim3(blocks), dim3(NTHREADS), 0, s, smooth_of(a), bx, partials);
    else
        hipLaunchKernelGGL(k_smooth_fwd<2>, dim3(blocks), dim3(NTHREADS), 0, s, smooth_of(a), bx, partials);
    hipLaunchKernelGGL(k_smooth_final, dim3(1), dim3(NTHREADS), 0, s, blocks, (double)a.height * (double)a.width, a.weight,
                       partials, a.out);
}

void launch_smooth_backward(const lr_smooth_args& a, hipStream_t s)
{
    const int blocks = blocks_of(a.height, a.width, SB_Y), bx = blocks_x_of(a.width);
    if (a.order == 1)
        hipLaunchKernelGGL(k_smooth_bwd<1>, dim3(blocks), dim3(NTHREADS), 0, s, smooth_of(a), bx, a.weight, a.upstream, a.dL_dmap);
    else
        hipLaunchKernelGGL(k_smooth_bwd<2>, dim3(blocks), dim3(NTHREADS), 0, s, smooth_of(a), bx, a.weight, a.upstream, a.dL_dmap);
}

}  // namespace lr
