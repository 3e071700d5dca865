// filter3d.hip -- the 3D smoothing filter of Mip-Splatting (Yu et al., "Mip-Splatting: Alias-free 3D Gaussian Splatting", 2024;
// luciddreamer_amd/filter3d.py, DESIGN.md section 4b-F3D, formulas in include/lucid_raster.h).  The filter acts on the STORED
// parameters (log scale [P,3], logit opacity [P,1]) before a rasterizer sees them; no rasterizer kernel knows about it.
//
//   sampling rate (lr_filter3d_update): d_k = min over the cameras that see Gaussian k of z / fx, filter_k = sqrt(variance) d_k.
//       k_filter3d_rate : one lane per Gaussian; the cameras (20 floats each) pass through LDS in chunks of F3_CAM_CHUNK, so V is
//                         unbounded and every lane reads a camera as an LDS broadcast.  A Gaussian no camera sees is marked
//                         with F3_UNSEEN in filter3D; the workgroup's largest d over its seen lanes goes to ws[blockIdx.x].
//       k_filter3d_fill : every workgroup takes the maximum of the ws entries (a few KB, from L2) and replaces the marks by
//                         sqrt(variance) * max d, or by 0 when nothing was seen.
//     min and max do not depend on the order: the result is bit-repeatable.  No float atomics, no copy to the host.
//   apply (lr_filter3d_apply_forward / _backward): s' = sqrt(s^2 + f^2), o' = o sqrt(prod s^2 / prod s'^2), in the stored or the
//     activated domain, 36 B per Gaussian forward and 52 B backward; the backward recomputes, nothing is saved.  The [P,3] rows
//     pass through LDS so that global loads and stores are contiguous dwords (lane i of a wave reads words i, i + 256, i + 512
//     of its workgroup's 768 and picks its own three at stride 3, which is conflict-free).
// This file is compiled with -ffp-contract=off: the visibility tests of k_filter3d_rate then are the float32 operations the
// header spells out, one rounding each, and a host restatement of them agrees to the bit.
#include "common.h"
#include <cmath>

namespace lr {

namespace {

constexpr int F3_THREADS = 256;
constexpr int F3_CAM_CHUNK = 64;            // cameras per LDS chunk: 64 x 20 floats = 5 KB
constexpr int F3_CAM_FLOATS = 20;           // 16 matrix floats (row-vector convention), fx, fy, W, H
constexpr float F3_UNSEEN = -1.0f;          // no d is negative: z > 0.2 and fx > 0
constexpr float F3_NEAR = 0.2f;             // the rasterizer's near cull
constexpr float F3_MARGIN = 0.65f;          // half the image extended by 15 % on every side

// maximum over the workgroup, in every thread; `red` holds F3_THREADS floats
__device__ __forceinline__ float block_max(float v, float* red)
{
    red[threadIdx.x] = v;
    lds_barrier();
    for (int s = F3_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        lds_barrier();
    }
    const float r = red[0];
    lds_barrier();
    return r;
}

__global__ void __launch_bounds__(F3_THREADS)
k_filter3d_rate(int P, int V, const float* __restrict__ means3D, const float* __restrict__ cams, float sqrt_variance,
                float* __restrict__ filter3D, unsigned char* __restrict__ seen_out, float* __restrict__ block_maxima)
{
    __shared__ float cam[F3_CAM_CHUNK * F3_CAM_FLOATS];
    __shared__ float red[F3_THREADS];
    const size_t i = (size_t)blockIdx.x * F3_THREADS + threadIdx.x;
    const bool live = i < (size_t)P;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) { x = means3D[3 * i]; y = means3D[3 * i + 1]; z = means3D[3 * i + 2]; }
    float d = F3_UNSEEN;
    for (int c0 = 0; c0 < V; c0 += F3_CAM_CHUNK) {
        const int n = min(F3_CAM_CHUNK, V - c0);
        for (int w = threadIdx.x; w < n * F3_CAM_FLOATS; w += F3_THREADS) cam[w] = cams[(size_t)c0 * F3_CAM_FLOATS + w];
        lds_barrier();
        for (int c = 0; c < n; c++) {
            const float* __restrict__ m = cam + c * F3_CAM_FLOATS;
            const float vx = ((m[0] * x + m[4] * y) + m[8] * z) + m[12];
            const float vy = ((m[1] * x + m[5] * y) + m[9] * z) + m[13];
            const float vz = ((m[2] * x + m[6] * y) + m[10] * z) + m[14];
            const float fx = m[16], fy = m[17];
            const bool in = vz > F3_NEAR && fabsf(vx / vz * fx) <= F3_MARGIN * m[18] && fabsf(vy / vz * fy) <= F3_MARGIN * m[19];
            if (in) {
                const float dc = vz / fx;
                d = d < 0.f ? dc : fminf(d, dc);
            }
        }
        lds_barrier();
    }
    const bool is_seen = live && d >= 0.f;
    if (live) {
        filter3D[i] = is_seen ? sqrt_variance * d : F3_UNSEEN;
        if (seen_out) seen_out[i] = is_seen ? 1 : 0;
    }
    const float m = block_max(is_seen ? d : F3_UNSEEN, red);
    if (threadIdx.x == 0) block_maxima[blockIdx.x] = m;
}

__global__ void __launch_bounds__(F3_THREADS)
k_filter3d_fill(int P, int n_maxima, const float* __restrict__ block_maxima, float sqrt_variance, float* __restrict__ filter3D)
{
    __shared__ float red[F3_THREADS];
    float m = F3_UNSEEN;
    for (int b = threadIdx.x; b < n_maxima; b += F3_THREADS) m = fmaxf(m, block_maxima[b]);
    m = block_max(m, red);
    const float fill = m >= 0.f ? sqrt_variance * m : 0.0f;
    for (size_t i = (size_t)blockIdx.x * F3_THREADS + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * F3_THREADS)
        if (filter3D[i] < 0.f) filter3D[i] = fill;
}

// ---- apply ------------------------------------------------------------------------------------------------------------------
// words [3 * base, 3 * base + 768) of a [P,3] tensor -> sh (zero beyond the tensor's end); the caller puts a barrier behind it
__device__ __forceinline__ void rows_to_lds(const float* __restrict__ src, size_t base, size_t n3, float* sh)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const size_t w = 3 * base + (size_t)(k * F3_THREADS) + threadIdx.x;
        sh[k * F3_THREADS + threadIdx.x] = w < n3 ? src[w] : 0.0f;
    }
}

__device__ __forceinline__ void lds_to_rows(const float* sh, size_t base, size_t n3, float* __restrict__ dst)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const size_t w = 3 * base + (size_t)(k * F3_THREADS) + threadIdx.x;
        if (w < n3) dst[w] = sh[k * F3_THREADS + threadIdx.x];
    }
}

// What forward and backward share of one Gaussian, from r[3], q, f (f > 0):
//   t_j = f^2 exp(-2 r_j);  h_j = log1p(t_j) / 2, or for t_j > 1 log f - r_j + log1p(1 / t_j) / 2 (finite for tiny scales)
//   u_j = 1 / (1 + t_j), w_j = 1 - u_j, each formed from min(t_j, 1 / t_j) without a subtraction
//   log c = -(h_0 + h_1 + h_2);  sig = sigmoid(q), nsig = sigmoid(-q), log_sig = log sigmoid(q), all from e = exp(-|q|)
//   one_minus_o = 1 - sig c = nsig + sig (-expm1(log c))
struct F3Terms {
    float h[3], u[3], w[3];
    float log_c, sig, nsig, log_sig, one_minus_o;
};

__device__ __forceinline__ F3Terms f3_terms(const float r[3], float q, float f)
{
    F3Terms T;
    const float f2 = f * f, log_f = logf(f);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        // one log1p and one reciprocal of 1 + m for both cases, m = min(t, 1 / t): selects instead of a divergent branch
        const float t = f2 * expf(-2.0f * r[j]);
        const bool small = t <= 1.0f;
        const float m = small ? t : 1.0f / t;
        const float half_lp = 0.5f * log1pf(m), inv = 1.0f / (1.0f + m);
        T.h[j] = small ? half_lp : (log_f - r[j]) + half_lp;
        T.u[j] = small ? inv : m * inv;
        T.w[j] = small ? m * inv : inv;
    }
    T.log_c = -((T.h[0] + T.h[1]) + T.h[2]);
    const float e = expf(-fabsf(q));
    const float inv = 1.0f / (1.0f + e);
    T.sig = q >= 0.f ? inv : e * inv;
    T.nsig = q >= 0.f ? e * inv : inv;
    T.log_sig = fminf(q, 0.f) - log1pf(e);
    T.one_minus_o = T.nsig + T.sig * (-expm1f(T.log_c));
    return T;
}

template <bool ACTIVATED>
__global__ void __launch_bounds__(F3_THREADS)
k_filter3d_apply_fwd(int P, const float* __restrict__ raw_scale, const float* __restrict__ raw_opacity,
                     const float* __restrict__ filter3D, float* __restrict__ out_scale, float* __restrict__ out_opacity)
{
    __shared__ float sh[3 * F3_THREADS];
    const size_t base = (size_t)blockIdx.x * F3_THREADS, i = base + threadIdx.x, n3 = 3 * (size_t)P;
    rows_to_lds(raw_scale, base, n3, sh);
    lds_barrier();
    const float r[3] = { sh[3 * threadIdx.x], sh[3 * threadIdx.x + 1], sh[3 * threadIdx.x + 2] };
    lds_barrier();
    float o[3] = { 0.f, 0.f, 0.f };
    if (i < (size_t)P) {
        const float q = raw_opacity[i], f = filter3D[i];
        float oo;
        if (!(f > 0.f)) {
            // no filter: the stored domain keeps its bits
            if (ACTIVATED) {
                for (int j = 0; j < 3; j++) o[j] = act_scale(r[j]);
                oo = act_opacity(q);
            } else {
                for (int j = 0; j < 3; j++) o[j] = r[j];
                oo = q;
            }
        } else {
            const F3Terms T = f3_terms(r, q, f);
            for (int j = 0; j < 3; j++) o[j] = ACTIVATED ? expf(r[j] + T.h[j]) : r[j] + T.h[j];
            oo = ACTIVATED ? T.sig * expf(T.log_c) : (T.log_sig + T.log_c) - logf(T.one_minus_o);
        }
        out_opacity[i] = oo;
    }
    sh[3 * threadIdx.x] = o[0]; sh[3 * threadIdx.x + 1] = o[1]; sh[3 * threadIdx.x + 2] = o[2];
    lds_barrier();
    lds_to_rows(sh, base, n3, out_scale);
}

template <bool ACTIVATED>
__global__ void __launch_bounds__(F3_THREADS)
k_filter3d_apply_bwd(int P, const float* __restrict__ raw_scale, const float* __restrict__ raw_opacity,
                     const float* __restrict__ filter3D, const float* __restrict__ g_scale, const float* __restrict__ g_opacity,
                     float* __restrict__ d_scale, float* __restrict__ d_opacity)
{
    __shared__ float sh[3 * F3_THREADS];
    __shared__ float sg[3 * F3_THREADS];
    const size_t base = (size_t)blockIdx.x * F3_THREADS, i = base + threadIdx.x, n3 = 3 * (size_t)P;
    rows_to_lds(raw_scale, base, n3, sh);
    if (g_scale) rows_to_lds(g_scale, base, n3, sg);
    lds_barrier();
    const float r[3] = { sh[3 * threadIdx.x], sh[3 * threadIdx.x + 1], sh[3 * threadIdx.x + 2] };
    float g[3] = { 0.f, 0.f, 0.f };
    if (g_scale) { g[0] = sg[3 * threadIdx.x]; g[1] = sg[3 * threadIdx.x + 1]; g[2] = sg[3 * threadIdx.x + 2]; }
    lds_barrier();
    float dr[3] = { 0.f, 0.f, 0.f };
    if (i < (size_t)P) {
        const float q = raw_opacity[i], f = filter3D[i];
        const float go = g_opacity ? g_opacity[i] : 0.0f;
        float dq;
        if (!(f > 0.f)) {
            if (ACTIVATED) {
                for (int j = 0; j < 3; j++) dr[j] = g[j] * act_scale(r[j]);
                const float s = act_opacity(q);
                dq = go * (s * (1.0f - s));
            } else {
                for (int j = 0; j < 3; j++) dr[j] = g[j];
                dq = go;
            }
        } else {
            const F3Terms T = f3_terms(r, q, f);
            if (ACTIVATED) {
                const float c = expf(T.log_c);
                const float o = T.sig * c;
                for (int j = 0; j < 3; j++) dr[j] = g[j] * expf(r[j] + T.h[j]) * T.u[j] + go * o * T.w[j];
                dq = go * c * (T.sig * T.nsig);
            } else {
                for (int j = 0; j < 3; j++) dr[j] = g[j] * T.u[j] + go * T.w[j] / T.one_minus_o;
                dq = go * T.nsig / T.one_minus_o;
            }
        }
        d_opacity[i] = dq;
    }
    sh[3 * threadIdx.x] = dr[0]; sh[3 * threadIdx.x + 1] = dr[1]; sh[3 * threadIdx.x + 2] = dr[2];
    lds_barrier();
    lds_to_rows(sh, base, n3, d_scale);
}

inline unsigned f3_blocks(int P) { return (unsigned)(((size_t)P + F3_THREADS - 1) / F3_THREADS); }

}  // namespace

size_t filter3d_workspace_bytes(int P) { return align_up((size_t)(P > 0 ? f3_blocks(P) : 1) * sizeof(float)); }

void launch_filter3d_update(int P, int V, const float* means3D, const float* cams, float variance, float* filter3D,
                            unsigned char* seen, char* ws, hipStream_t s)
{
    const float sqrt_variance = sqrtf(variance);
    float* maxima = reinterpret_cast<float*>(ws);
    const unsigned nb = f3_blocks(P);
    hipLaunchKernelGGL(k_filter3d_rate, dim3(nb), dim3(F3_THREADS), 0, s, P, V, means3D, cams, sqrt_variance, filter3D, seen, maxima);
    hipLaunchKernelGGL(k_filter3d_fill, dim3(nb < 1024u ? nb : 1024u), dim3(F3_THREADS), 0, s, P, (int)nb, maxima, sqrt_variance,
                       filter3D);
}

void launch_filter3d_apply_forward(int P, const float* raw_scale, const float* raw_opacity, const float* filter3D, bool activated,
                                   float* out_scale, float* out_opacity, hipStream_t s)
{
    const dim3 grid(f3_blocks(P)), block(F3_THREADS);
    if (activated)
        hipLaunchKernelGGL(k_filter3d_apply_fwd<true>, grid, block, 0, s, P, raw_scale, raw_opacity, filter3D, out_scale, out_opacity);
    else
        hipLaunchKernelGGL(k_filter3d_apply_fwd<false>, grid, block, 0, s, P, raw_scale, raw_opacity, filter3D, out_scale, out_opacity);
}

void launch_filter3d_apply_backward(int P, const float* raw_scale, const float* raw_opacity, const float* filter3D, bool activated,
                                    const float* g_scale, const float* g_opacity, float* d_scale, float* d_opacity, hipStream_t s)
{
    const dim3 grid(f3_blocks(P)), block(F3_THREADS);
    if (activated)
        hipLaunchKernelGGL(k_filter3d_apply_bwd<true>, grid, block, 0, s, P, raw_scale, raw_opacity, filter3D, g_scale, g_opacity,
                           d_scale, d_opacity);
    else
        hipLaunchKernelGGL(k_filter3d_apply_bwd<false>, grid, block, 0, s, P, raw_scale, raw_opacity, filter3D, g_scale, g_opacity,
                           d_scale, d_opacity);
}

}  // namespace lr
