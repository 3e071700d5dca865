// loss.hip -- fused L1 + DSSIM photometric loss and its gradient for gfx950.
//
// Replaces, for the training loop's loss (R/luciddreamer.py:301-304)
//     loss = (1 - lambda) * l1_loss(image, gt) + lambda * (1 - ssim(image, gt))
// the reference's Python composition (R/utils/loss.py:18-69): five grouped 11x11 F.conv2d (121 taps each, the 2-D
// window is the outer product of a normalised 1-D Gaussian, sigma 1.5, zero padding 5), a dozen elementwise
// kernels, two reductions, and the autograd replay of all of it.  Here:
//   k_ssim_fwd : one pass over the image pair.  A 256-thread workgroup owns a 32x32 tile of one channel, stages
//                the 42x42 halo region of both images in LDS, runs the five window sums SEPARABLY (11 + 11 taps,
//                four adjacent outputs per thread per pass so that the sliding window re-uses LDS reads), forms the
//                SSIM value and the three partial derivatives dS/d(conv I), dS/d(conv I^2), dS/d(conv I*G) per
//                pixel, writes those three maps, and reduces sum(S) and sum|I-G| per workgroup (fixed order).
//   k_loss_final: sums the per-workgroup partials in a fixed order (double) -> {loss, l1, ssim}.
//   k_ssim_bwd : the adjoint of a symmetric zero-padded window sum is the same window sum, so
//                dL/dI(q) = -lambda/n * [ W*D1 + 2 I(q) W*D2 + G(q) W*D3 ](q) + (1-lambda)/n * sign(I-G)(q),
//                again separable through LDS, times the upstream scalar (device pointer, no host sync).
// HBM-bound by construction: ~60 B per pixel-channel over both passes; no atomics, deterministic.
// k_ssim_fwd_masked / k_ssim_bwd_masked (lr_masked_l1_dssim_*): the same bodies (loss_ssim_*_body.h) on the masked pair
// (m I, m G), m a content mask [H,W]; 4 B more per pixel-channel and pass.  Below them: the masked depth L1 and the alpha hole
// term, elementwise passes with fixed-order double reductions, and the Pearson depth loss (k_depth_pearson_*), whose sums are
// double from the pixel on.
#include "common.h"
#include <cmath>

namespace lr {

namespace {

constexpr int LT = 32;                 // tile edge (outputs)
constexpr int HALO = 5;                // window 11
constexpr int LR_IN = LT + 2 * HALO;   // 42
constexpr int LTHREADS = 256;
constexpr int NSTAGE = (LR_IN * LR_IN + LTHREADS - 1) / LTHREADS;   // halo elements staged per thread (7)

struct Win { float w[11]; };

// gaussian(11, 1.5) of R/utils/loss.py:26-28: exp in double, cast to float32, normalised in float32
Win make_window()
{
    Win g;
    float v[11], sum = 0.f;
    for (int x = 0; x < 11; x++) { v[x] = (float)std::exp(-(double)((x - 5) * (x - 5)) / (2.0 * 1.5 * 1.5)); sum += v[x]; }
    for (int x = 0; x < 11; x++) g.w[x] = v[x] / sum;
    return g;
}

// Workgroups are dealt to the 8 XCDs round robin (blockIdx % 8) and each XCD has its own L2.  Neighbouring tiles share
// their halo rows, so every XCD gets a contiguous run of tiles (a band of the image): with the plain order the halo
// lines were fetched from HBM once per XCD that touched them (k_ssim_bwd: 339 MB fetched for 125 MB of maps).
// Returns the logical block (tile + channel * tiles) of this workgroup or -1 (grid padded to a multiple of 8).
__device__ __forceinline__ int xcd_band_block(int n_blocks)
{
    const int per_xcd = (n_blocks + 7) >> 3;
    const int lb = (int)(blockIdx.x & 7u) * per_xcd + (int)(blockIdx.x >> 3);
    return ((int)(blockIdx.x >> 3) < per_xcd && lb < n_blocks) ? lb : -1;
}

__device__ __forceinline__ float block_sum(float v, float* s_tmp)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int w = threadIdx.x >> 6;
    lds_barrier();
    if ((threadIdx.x & 63) == 0) s_tmp[w] = v;
    lds_barrier();
    return s_tmp[0] + s_tmp[1] + s_tmp[2] + s_tmp[3];
}


__global__ void __launch_bounds__(LTHREADS)
k_ssim_fwd(int H, int W, int tiles_x, int tiles_y, Win win, const float* __restrict__ img, const float* __restrict__ gt,
           float* __restrict__ D1, float* __restrict__ D2, float* __restrict__ D3, float2* __restrict__ partials,
           int n_blocks)
{
    constexpr bool MASKED = false;
    const float* const mask = nullptr;
#include "loss_ssim_fwd_body.h"
}

__global__ void __launch_bounds__(LTHREADS)
k_ssim_fwd_masked(int H, int W, int tiles_x, int tiles_y, Win win, const float* __restrict__ img, const float* __restrict__ gt,
                  const float* __restrict__ mask, float* __restrict__ D1, float* __restrict__ D2, float* __restrict__ D3,
                  float2* __restrict__ partials, int n_blocks)
{
    constexpr bool MASKED = true;
#include "loss_ssim_fwd_body.h"
}

// {loss, l1, ssim} from the per-workgroup partials, fixed order, one workgroup of LTHREADS threads
__device__ __forceinline__ void loss_final(int n_blocks, double n_elems, float lambda, const float2* __restrict__ partials,
                                           float* __restrict__ out, double* s_a, double* s_b)
{
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += LTHREADS) { const float2 p = partials[i]; a += p.x; b += p.y; }
    s_a[threadIdx.x] = a; s_b[threadIdx.x] = b;
    lds_barrier();
    for (int off = LTHREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { s_a[threadIdx.x] += s_a[threadIdx.x + off]; s_b[threadIdx.x] += s_b[threadIdx.x + off]; }
        lds_barrier();
    }
    if (threadIdx.x == 0) {
        const float ssim = (float)(s_a[0] / n_elems), l1 = (float)(s_b[0] / n_elems);
        out[0] = (1.0f - lambda) * l1 + lambda * (1.0f - ssim);
        out[1] = l1;
        out[2] = ssim;
    }
}

__global__ void __launch_bounds__(LTHREADS)
k_loss_final(int n_blocks, double n_elems, float lambda, const float2* __restrict__ partials, float* __restrict__ out)
{
    __shared__ double s_a[LTHREADS], s_b[LTHREADS];
    loss_final(n_blocks, n_elems, lambda, partials, out, s_a, s_b);
}


__global__ void __launch_bounds__(LTHREADS)
k_ssim_bwd(int H, int W, int tiles_x, int tiles_y, Win win, float lambda, float inv_n, const float* __restrict__ upstream,
           const float* __restrict__ w_ssim, const float* __restrict__ img, const float* __restrict__ gt, const float* __restrict__ D1,
           const float* __restrict__ D2, const float* __restrict__ D3, float* __restrict__ grad,
           const float2* __restrict__ partials, int n_blocks, double n_elems, float* __restrict__ out3)
{
    constexpr bool MASKED = false;
    const float* const mask = nullptr;
#include "loss_ssim_bwd_body.h"
}

__global__ void __launch_bounds__(LTHREADS)
k_ssim_bwd_masked(int H, int W, int tiles_x, int tiles_y, Win win, float lambda, float inv_n, const float* __restrict__ upstream,
                  const float* __restrict__ w_ssim, const float* __restrict__ img, const float* __restrict__ gt,
                  const float* __restrict__ mask, const float* __restrict__ D1, const float* __restrict__ D2,
                  const float* __restrict__ D3, float* __restrict__ grad, const float2* __restrict__ partials, int n_blocks,
                  double n_elems, float* __restrict__ out3)
{
    constexpr bool MASKED = true;
#include "loss_ssim_bwd_body.h"
}

// ---- masked depth L1 (supervision of the rendered depth against a depth map, e.g. a monocular estimate) -------------------
//     loss = weight * mean_{H*W}( |depth - target| * [target > 0] ),   d loss / d depth = weight * sign(depth - target) * [target > 0] / (H*W)
// A target that is not > 0 (no estimate, NaN) contributes nothing: the masked pixels are SELECTED away, so a NaN target never
// reaches the sum or the gradient.  HBM-bound (12 B per pixel over both passes); deterministic: fixed per-workgroup
// partial sums, reduced in a fixed order in double; no atomics.
constexpr int DL_ITEMS = 8;                          // pixels per thread
constexpr int DL_BLOCK = LTHREADS * DL_ITEMS;        // pixels per workgroup (2048)

__device__ __forceinline__ double block_sum_d(double v, double* s_tmp)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_tmp[w] = v;
    lds_barrier();
    return (s_tmp[0] + s_tmp[1]) + (s_tmp[2] + s_tmp[3]);
}

__global__ void __launch_bounds__(LTHREADS)
k_depth_l1_fwd(int n, const float* __restrict__ depth, const float* __restrict__ target, double* __restrict__ partials)
{
    __shared__ double s_tmp[4];
    const int base = (int)blockIdx.x * DL_BLOCK + (int)threadIdx.x;
    float d[DL_ITEMS], t[DL_ITEMS];
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) {             // all loads first; pixel base + 256 i: coalesced
        const int q = base + i * LTHREADS;
        const bool ok = q < n;
        d[i] = ok ? depth[q] : 0.f;
        t[i] = ok ? target[q] : 0.f;
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) sum += t[i] > 0.f ? fabsf(d[i] - t[i]) : 0.f;
    const double bs = block_sum_d((double)sum, s_tmp);
    if (threadIdx.x == 0) partials[blockIdx.x] = bs;
}

// {weight * mean, mean} of the partials, fixed order; fused step (out_losses of lr_views_accumulate with depth_targets): the colour
// loss already in out[0] gets the weighted depth term added, the unweighted mean goes to out[3]
__device__ __forceinline__ void depth_l1_final(int n_blocks, double n_elems, float weight, const double* __restrict__ partials,
                                               float* __restrict__ out, bool fused, double* s_a)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += LTHREADS) a += partials[i];
    s_a[threadIdx.x] = a;
    lds_barrier();
    for (int off = LTHREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_a[threadIdx.x] += s_a[threadIdx.x + off];
        lds_barrier();
    }
    if (threadIdx.x == 0) {
        const float mean = (float)(s_a[0] / n_elems);
        if (fused) { if (weight != 0.f) out[0] = out[0] + weight * mean; out[3] = mean; }
        else { out[0] = weight * mean; }
    }
}

__global__ void __launch_bounds__(LTHREADS)
k_depth_l1_final(int n_blocks, double n_elems, float weight, const double* __restrict__ partials, float* __restrict__ out,
                 int fused)
{
    __shared__ double s_a[LTHREADS];
    depth_l1_final(n_blocks, n_elems, weight, partials, out, fused != 0, s_a);
}

// dL/ddepth = (upstream * weight) / n * sign(depth - target) * [target > 0]: the product, divided, is what torch's autograd of
// the definition forms (mul backward, then mean backward's division), so the gradient is bit-equal to it.  fused_out: the
// fused step's loss value (depth_l1_final) rides in workgroup 0, one launch less per view.
__global__ void __launch_bounds__(LTHREADS)
k_depth_l1_bwd(int n, float weight, const float* __restrict__ upstream, const float* __restrict__ depth,
               const float* __restrict__ target, float* __restrict__ grad, const double* __restrict__ partials, int n_blocks,
               float* __restrict__ fused_out)
{
    if (fused_out != nullptr && blockIdx.x == 0) {
        __shared__ double s_a[LTHREADS];
        depth_l1_final(n_blocks, (double)n, weight, partials, fused_out, true, s_a);
    }
    const float up = upstream != nullptr ? upstream[0] : 1.0f;
    const float k = (up * weight) / (float)n;
    const int base = (int)blockIdx.x * DL_BLOCK + (int)threadIdx.x;
    float d[DL_ITEMS], t[DL_ITEMS];
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) {
        const int q = base + i * LTHREADS;
        const bool ok = q < n;
        d[i] = ok ? depth[q] : 0.f;
        t[i] = ok ? target[q] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) {
        const int q = base + i * LTHREADS;
        if (q < n) {
            const float r = d[i] - t[i];
            const float sgn = r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f);       // torch.abs backward: sign, 0 at 0
            grad[q] = t[i] > 0.f ? sgn * k : 0.f;
        }
    }
}

// ---- alpha hole term (coverage where the target frame has no content) -----------------------------------------------------
//     loss = weight * mean_{H*W}( A * (1 - m) ),   d loss / d A = weight * (1 - m) / (H*W)
// A = 1 - T_final, the alpha output; m [H,W] the content mask in [0, 1].  The forward reads A -- or T_final itself, from_T, and
// forms A = 1 - T_final as lr_render_alpha does, writing it to alpha_out when the caller keeps the alpha image.  Partials,
// fixed-order double reduction and the value formed by the final kernel or by the backward (LossValue) as k_depth_l1_*; the
// row slot is out[4].
__global__ void __launch_bounds__(LTHREADS)
k_alpha_hole_fwd(int n, const float* __restrict__ src, int from_T, const float* __restrict__ mask, double* __restrict__ partials,
                 float* __restrict__ alpha_out)
{
    __shared__ double s_tmp[4];
    const int base = (int)blockIdx.x * DL_BLOCK + (int)threadIdx.x;
    float a[DL_ITEMS], m[DL_ITEMS];
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) {             // all loads first; pixel base + 256 i: coalesced
        const int q = base + i * LTHREADS;
        const bool ok = q < n;
        a[i] = ok ? src[q] : (from_T ? 1.f : 0.f);
        m[i] = ok ? mask[q] : 1.f;
    }
    if (from_T) {
#pragma unroll
        for (int i = 0; i < DL_ITEMS; i++) a[i] = 1.0f - a[i];
        if (alpha_out != nullptr) {
#pragma unroll
            for (int i = 0; i < DL_ITEMS; i++) {
                const int q = base + i * LTHREADS;
                if (q < n) alpha_out[q] = a[i];
            }
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) sum += a[i] * (1.0f - m[i]);
    const double bs = block_sum_d((double)sum, s_tmp);
    if (threadIdx.x == 0) partials[blockIdx.x] = bs;
}

// as depth_l1_final, with the fused step's unweighted mean in out[4] (out_losses of lr_views_accumulate with masks);
// fused 2: a step without a depth term, whose depth_l1 out[3] is reported as 0
__device__ __forceinline__ void alpha_hole_final(int n_blocks, double n_elems, float weight, const double* __restrict__ partials,
                                                 float* __restrict__ out, int fused, double* s_a)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += LTHREADS) a += partials[i];
    s_a[threadIdx.x] = a;
    lds_barrier();
    for (int off = LTHREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_a[threadIdx.x] += s_a[threadIdx.x + off];
        lds_barrier();
    }
    if (threadIdx.x == 0) {
        const float mean = (float)(s_a[0] / n_elems);
        if (fused) {
            if (weight != 0.f) out[0] = out[0] + weight * mean;
            out[4] = mean;
            if (fused == 2) out[3] = 0.f;
        } else {
            out[0] = weight * mean;
        }
    }
}

__global__ void __launch_bounds__(LTHREADS)
k_alpha_hole_final(int n_blocks, double n_elems, float weight, const double* __restrict__ partials, float* __restrict__ out,
                   int fused)
{
    __shared__ double s_a[LTHREADS];
    alpha_hole_final(n_blocks, n_elems, weight, partials, out, fused, s_a);
}

// dL/dA = (upstream * weight) / n * (1 - m): torch's autograd of the definition (mul, mean backward's division, then the
// product with 1 - m), bit for bit.  It does not depend on A.  fused_out: the fused step's value rides in workgroup 0.
__global__ void __launch_bounds__(LTHREADS)
k_alpha_hole_bwd(int n, float weight, const float* __restrict__ upstream, const float* __restrict__ mask,
                 float* __restrict__ grad, const double* __restrict__ partials, int n_blocks, float* __restrict__ fused_out,
                 int fused)
{
    if (fused_out != nullptr && blockIdx.x == 0) {
        __shared__ double s_a[LTHREADS];
        alpha_hole_final(n_blocks, (double)n, weight, partials, fused_out, fused, s_a);
    }
    const float up = upstream != nullptr ? upstream[0] : 1.0f;
    const float k = (up * weight) / (float)n;
    const int base = (int)blockIdx.x * DL_BLOCK + (int)threadIdx.x;
    float m[DL_ITEMS];
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) {
        const int q = base + i * LTHREADS;
        m[i] = q < n ? mask[q] : 1.f;
    }
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) {
        const int q = base + i * LTHREADS;
        if (q < n) grad[q] = k * (1.0f - m[i]);
    }
}

// ---- Pearson depth loss (scale- and shift-invariant supervision of the rendered depth by an estimated depth map) ------------
// The valid set is M = {i : target_i > 0}, exactly the masked depth L1's (NaN targets and targets <= 0 are excluded; excluded
// pixels are SELECTED away, never multiplied), m = |M|.  All sums run over M, in double:
//     Sd = sum d, St = sum t, Sdd = sum d^2, Stt = sum t^2, Sdt = sum d t
//     mu_d = Sd / m, mu_t = St / m
//     Sxx = Sdd - Sd^2 / m, Syy = Stt - St^2 / m, Sxy = Sdt - Sd St / m
//     rho = Sxy / sqrt(Sxx Syy), clamped to [-1, 1];  term = 1 - rho, loss = weight * term
//     for i in M: dloss/dd_i = -weight * ( (t_i - mu_t) / sqrt(Sxx Syy) - rho (d_i - mu_d) / Sxx ), 0 outside M
// (the mean-subtraction terms cancel exactly, so the backward is elementwise once mu_d, mu_t, 1 / sqrt(Sxx Syy), rho / Sxx and
// upstream * weight are known).  Degenerate inputs -- m < 2, Sxx <= 1e-12 Sdd or Syy <= 1e-12 Stt (a non-finite sum is neither
// > anything) -- have no correlation: term = 0, loss = 0, rho = 0 and the gradient is exactly zero everywhere.  1e-12 sits
// four orders of magnitude above the double-precision cancellation error of the one-pass variance.
// Every pixel's d and t are converted to double BEFORE any product or sum is formed; per-lane, per-workgroup and final sums
// are double, in a fixed order, no atomics: the value is bit-repeatable.  (A float sum of d^2 loses the variance of a distant,
// flat depth map.)  HBM-bound like the L1 pair: 8 B per pixel forward, 8 + 4 backward; the fp64 FMAs hide under that.
//   k_depth_pearson_fwd  : six partials per workgroup {Sd, St, Sdd, Stt, Sdt, m}
//   k_depth_pearson_final: one workgroup; reduces the partials, decides degeneracy, writes the coefficient record and the value(s)
//   k_depth_pearson_bwd  : one elementwise pass that reads the record (every workgroup needs the coefficients: it must not
//                          re-reduce the partials itself, unlike the L1 backward whose constant needs no sum)
constexpr int DP_SUMS = 6;
// the coefficient record behind the partials (doubles): what the backward and the callers read
enum { DP_MU_D = 0, DP_MU_T = 1, DP_INV_NORM = 2, DP_RHO_OVER_SXX = 3, DP_TERM = 4, DP_RHO = 5, DP_RECORD = 8 };

__global__ void __launch_bounds__(LTHREADS)
k_depth_pearson_fwd(int n, const float* __restrict__ depth, const float* __restrict__ target, double* __restrict__ partials)
{
    __shared__ double s_tmp[4][DP_SUMS];
    const int base = (int)blockIdx.x * DL_BLOCK + (int)threadIdx.x;
    float d[DL_ITEMS], t[DL_ITEMS];
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) {             // all loads first; pixel base + 256 i: coalesced
        const int q = base + i * LTHREADS;
        const bool ok = q < n;
        d[i] = ok ? depth[q] : 0.f;
        t[i] = ok ? target[q] : 0.f;
    }
    double s[DP_SUMS] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) {
        const bool valid = t[i] > 0.f;
        const double dd = valid ? (double)d[i] : 0.0, tt = valid ? (double)t[i] : 0.0;
        s[0] += dd; s[1] += tt; s[2] += dd * dd; s[3] += tt * tt; s[4] += dd * tt; s[5] += valid ? 1.0 : 0.0;
    }
#pragma unroll
    for (int j = 0; j < DP_SUMS; j++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_xor(s[j], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < DP_SUMS; j++) s_tmp[threadIdx.x >> 6][j] = s[j];
    }
    lds_barrier();
    if (threadIdx.x < DP_SUMS)
        partials[(size_t)blockIdx.x * DP_SUMS + threadIdx.x] =
            (s_tmp[0][threadIdx.x] + s_tmp[1][threadIdx.x]) + (s_tmp[2][threadIdx.x] + s_tmp[3][threadIdx.x]);
}

// fused 0: out = {weight * term, rho}; fused 1 (out = the view's {loss, l1, ssim, depth term} of lr_views_accumulate, the colour
// loss already in out[0]): out[0] += weight * term when weight != 0, out[3] = term -- what depth_l1_final does in fused mode
__global__ void __launch_bounds__(LTHREADS)
k_depth_pearson_final(int n_blocks, float weight, const double* __restrict__ partials, double* __restrict__ record,
                      float* __restrict__ out, int fused)
{
    __shared__ double s_a[DP_SUMS][LTHREADS];
    double a[DP_SUMS] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int i = threadIdx.x; i < n_blocks; i += LTHREADS) {
#pragma unroll
        for (int j = 0; j < DP_SUMS; j++) a[j] += partials[(size_t)i * DP_SUMS + j];
    }
#pragma unroll
    for (int j = 0; j < DP_SUMS; j++) s_a[j][threadIdx.x] = a[j];
    lds_barrier();
    for (int off = LTHREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
#pragma unroll
            for (int j = 0; j < DP_SUMS; j++) s_a[j][threadIdx.x] += s_a[j][threadIdx.x + off];
        }
        lds_barrier();
    }
    if (threadIdx.x == 0) {
        const double Sd = s_a[0][0], St = s_a[1][0], Sdd = s_a[2][0], Stt = s_a[3][0], Sdt = s_a[4][0], m = s_a[5][0];
        double mu_d = 0.0, mu_t = 0.0, inv_norm = 0.0, rho_over_sxx = 0.0, rho = 0.0;
        if (m >= 2.0) {
            const double Sxx = Sdd - Sd * Sd / m, Syy = Stt - St * St / m, Sxy = Sdt - Sd * St / m;
            if (Sxx > 1e-12 * Sdd && Syy > 1e-12 * Stt) {          // false for non-finite sums as well
                mu_d = Sd / m; mu_t = St / m;
                inv_norm = 1.0 / sqrt(Sxx * Syy);
                rho = fmin(fmax(Sxy * inv_norm, -1.0), 1.0);
                rho_over_sxx = rho / Sxx;
            }
        }
        const bool live = inv_norm > 0.0 && inv_norm <= 1.79769313486231570e308;      // an overflowed product is degenerate too
        if (!live) { mu_d = mu_t = inv_norm = rho_over_sxx = rho = 0.0; }
        const double term = live ? 1.0 - rho : 0.0;
        record[DP_MU_D] = mu_d; record[DP_MU_T] = mu_t; record[DP_INV_NORM] = inv_norm; record[DP_RHO_OVER_SXX] = rho_over_sxx;
        record[DP_TERM] = term; record[DP_RHO] = rho; record[6] = m; record[7] = 0.0;
        if (fused) { if (weight != 0.f) out[0] = out[0] + weight * (float)term; out[3] = (float)term; }
        else { out[0] = (float)((double)weight * term); out[1] = (float)rho; }
    }
}

// dL/dd_i = -(upstream * weight) * ( (t_i - mu_t) / sqrt(Sxx Syy) - (rho / Sxx) (d_i - mu_d) ) on M, in double, rounded to float
// once; a degenerate record (both coefficients 0) writes exact zeros whatever the pixels hold
__global__ void __launch_bounds__(LTHREADS)
k_depth_pearson_bwd(int n, float weight, const float* __restrict__ upstream, const float* __restrict__ depth,
                    const float* __restrict__ target, const double* __restrict__ record, float* __restrict__ grad)
{
    const int base = (int)blockIdx.x * DL_BLOCK + (int)threadIdx.x;
    float d[DL_ITEMS], t[DL_ITEMS];
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) {
        const int q = base + i * LTHREADS;
        const bool ok = q < n;
        d[i] = ok ? depth[q] : 0.f;
        t[i] = ok ? target[q] : 0.f;
    }
    const double mu_d = record[DP_MU_D], mu_t = record[DP_MU_T], c_t = record[DP_INV_NORM], c_d = record[DP_RHO_OVER_SXX];
    const bool live = c_t != 0.0;
    const double k = -((double)(upstream != nullptr ? upstream[0] : 1.0f) * (double)weight);
#pragma unroll
    for (int i = 0; i < DL_ITEMS; i++) {
        const int q = base + i * LTHREADS;
        if (q < n) {
            const double g = k * (((double)t[i] - mu_t) * c_t - c_d * ((double)d[i] - mu_d));
            grad[q] = (live && t[i] > 0.f) ? (float)g : 0.f;
        }
    }
}

}  // namespace

size_t loss_workspace_bytes(int C, int H, int W)
{
    const size_t n = (size_t)C * H * W;
    const size_t blocks = (size_t)C * ((W + LT - 1) / LT) * ((H + LT - 1) / LT);
    return align_up(3 * n * sizeof(float)) + align_up(blocks * sizeof(float2));
}

void launch_loss_forward(const LossPair& p, LossValue value, hipStream_t s)
{
    static const Win win = make_window();
    const int H = p.H, W = p.W;
    const size_t n = (size_t)p.C * H * W;
    const int tx = (W + LT - 1) / LT, ty = (H + LT - 1) / LT;
    const int blocks = p.C * tx * ty;
    float* D = reinterpret_cast<float*>(p.ws);
    float2* partials = reinterpret_cast<float2*>(p.ws + align_up(3 * n * sizeof(float)));
    if (p.mask != nullptr)
        hipLaunchKernelGGL(k_ssim_fwd_masked, dim3((blocks + 7) / 8 * 8), dim3(LTHREADS), 0, s, H, W, tx, ty, win, p.img, p.gt,
                           p.mask, D, D + n, D + 2 * n, partials, blocks);
    else
        hipLaunchKernelGGL(k_ssim_fwd, dim3((blocks + 7) / 8 * 8), dim3(LTHREADS), 0, s, H, W, tx, ty, win, p.img, p.gt, D, D + n,
                           D + 2 * n, partials, blocks);
    if (value.where != LOSS_ROW_BY_BACKWARD)     // the pair's three floats lead the row: one final kernel for value and row
        hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(LTHREADS), 0, s, blocks, (double)n, p.lambda, partials, value.out);
}

void launch_loss_backward(const LossPair& p, const float* upstream, const float* w_ssim, float* grad, LossValue value,
                          hipStream_t s)
{
    static const Win win = make_window();
    const int H = p.H, W = p.W;
    const size_t n = (size_t)p.C * H * W;
    const int tx = (W + LT - 1) / LT, ty = (H + LT - 1) / LT;
    const int blocks = p.C * tx * ty;
    const float* D = reinterpret_cast<const float*>(p.ws);
    const float2* partials = reinterpret_cast<const float2*>(p.ws + align_up(3 * n * sizeof(float)));
    if (p.mask != nullptr)
        hipLaunchKernelGGL(k_ssim_bwd_masked, dim3((blocks + 7) / 8 * 8), dim3(LTHREADS), 0, s, H, W, tx, ty, win, p.lambda,
                           (float)(1.0 / (double)n), upstream, w_ssim, p.img, p.gt, p.mask, D, D + n, D + 2 * n, grad, partials,
                           blocks, (double)n, value.by_backward());
    else
        hipLaunchKernelGGL(k_ssim_bwd, dim3((blocks + 7) / 8 * 8), dim3(LTHREADS), 0, s, H, W, tx, ty, win, p.lambda,
                           (float)(1.0 / (double)n), upstream, w_ssim, p.img, p.gt, D, D + n, D + 2 * n, grad, partials, blocks,
                           (double)n, value.by_backward());
}

}  // namespace lr

namespace lr {

size_t depth_l1_workspace_bytes(int H, int W)
{
    const size_t n = (size_t)H * W;
    return align_up(((n + DL_BLOCK - 1) / DL_BLOCK) * sizeof(double));
}

void launch_depth_l1_forward(int H, int W, const float* depth, const float* target, float weight, char* ws, LossValue value,
                             hipStream_t s)
{
    const int n = H * W;
    const int blocks = (n + DL_BLOCK - 1) / DL_BLOCK;
    double* partials = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(k_depth_l1_fwd, dim3(blocks), dim3(LTHREADS), 0, s, n, depth, target, partials);
    if (value.where != LOSS_ROW_BY_BACKWARD)
        hipLaunchKernelGGL(k_depth_l1_final, dim3(1), dim3(LTHREADS), 0, s, blocks, (double)n, weight, partials, value.out,
                           value.where == LOSS_ROW ? 1 : 0);
}

void launch_depth_l1_backward(int H, int W, const float* depth, const float* target, float weight, const float* upstream,
                              const char* ws, float* grad, LossValue value, hipStream_t s)
{
    const int n = H * W;
    const int blocks = (n + DL_BLOCK - 1) / DL_BLOCK;
    hipLaunchKernelGGL(k_depth_l1_bwd, dim3(blocks), dim3(LTHREADS), 0, s, n, weight, upstream, depth, target, grad,
                       reinterpret_cast<const double*>(ws), blocks, value.by_backward());
}

}  // namespace lr

namespace lr {

// the partials [workgroups][6] and, behind them, the coefficient record
static size_t depth_pearson_record_offset(int H, int W)
{
    const size_t n = (size_t)H * W;
    return align_up(((n + DL_BLOCK - 1) / DL_BLOCK) * DP_SUMS * sizeof(double));
}

size_t depth_pearson_workspace_bytes(int H, int W)
{
    return depth_pearson_record_offset(H, W) + align_up(DP_RECORD * sizeof(double));
}

void launch_depth_pearson_forward(int H, int W, const float* depth, const float* target, float weight, char* ws, LossValue value,
                                  hipStream_t s)
{
    const int n = H * W;
    const int blocks = (n + DL_BLOCK - 1) / DL_BLOCK;
    double* partials = reinterpret_cast<double*>(ws);
    double* record = reinterpret_cast<double*>(ws + depth_pearson_record_offset(H, W));
    hipLaunchKernelGGL(k_depth_pearson_fwd, dim3(blocks), dim3(LTHREADS), 0, s, n, depth, target, partials);
    hipLaunchKernelGGL(k_depth_pearson_final, dim3(1), dim3(LTHREADS), 0, s, blocks, weight, partials, record, value.out,
                       value.where == LOSS_VALUE ? 0 : 1);
}

void launch_depth_pearson_backward(int H, int W, const float* depth, const float* target, float weight, const float* upstream,
                                   const char* ws, float* grad, hipStream_t s)
{
    const int n = H * W;
    const int blocks = (n + DL_BLOCK - 1) / DL_BLOCK;
    hipLaunchKernelGGL(k_depth_pearson_bwd, dim3(blocks), dim3(LTHREADS), 0, s, n, weight, upstream, depth, target,
                       reinterpret_cast<const double*>(ws + depth_pearson_record_offset(H, W)), grad);
}

}  // namespace lr

namespace lr {

size_t alpha_hole_workspace_bytes(int H, int W) { return depth_l1_workspace_bytes(H, W); }

void launch_alpha_hole_forward(int H, int W, const float* src, bool from_T, float* alpha_out, const float* mask, float weight,
                               char* ws, LossValue value, hipStream_t s)
{
    const int n = H * W;
    const int blocks = (n + DL_BLOCK - 1) / DL_BLOCK;
    double* partials = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(k_alpha_hole_fwd, dim3(blocks), dim3(LTHREADS), 0, s, n, src, from_T ? 1 : 0, mask, partials,
                       from_T ? alpha_out : nullptr);
    if (value.where != LOSS_ROW_BY_BACKWARD)
        hipLaunchKernelGGL(k_alpha_hole_final, dim3(1), dim3(LTHREADS), 0, s, blocks, (double)n, weight, partials, value.out,
                           value.where == LOSS_ROW ? (value.row_has_depth ? 1 : 2) : 0);
}

void launch_alpha_hole_backward(int H, int W, const float* mask, float weight, const float* upstream, const char* ws, float* grad,
                                LossValue value, hipStream_t s)
{
    const int n = H * W;
    const int blocks = (n + DL_BLOCK - 1) / DL_BLOCK;
    hipLaunchKernelGGL(k_alpha_hole_bwd, dim3(blocks), dim3(LTHREADS), 0, s, n, weight, upstream, mask, grad,
                       reinterpret_cast<const double*>(ws), blocks, value.by_backward(), value.row_has_depth ? 1 : 2);
}

}  // namespace lr
