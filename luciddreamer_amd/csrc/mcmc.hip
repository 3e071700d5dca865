// mcmc.hip -- the per-row kernels of the MCMC densification strategy (Kheradmand et al., "3D Gaussian Splatting as Markov
// Chain Monte Carlo", 2024; luciddreamer_amd/mcmc.py).  All inputs are the STORED GaussianModel
// parameters: logit opacity [P,1], log scale [P,3], unnormalised quaternion [P,4] in (r,x,y,z) order.
//
//   relocation / growth (lr_mcmc_relocate): n pairs (dst[j], src[j]); source i sampled c[i] times splits into N = min(c[i] + 1,
//     n_max) Gaussians of opacity o' = 1 - (1 - o)^(1/N) and scale s' = s o / den(o', N), the paper's eq. 9; every destination
//     becomes a copy of its source with the new opacity and scale; the Adam moments of every touched row are zeroed.
//       k_mcmc_count   : c[src[j]] += 1                       (integer atomics: the counts do not depend on the arrival order)
//       k_mcmc_compute : staged[j] = {logit o', log s'} from the source's OLD values.  One thread per PAIR: the threads of a
//                        source sampled several times compute the same bits from the same inputs and nothing is written to a
//                        parameter tensor in this kernel, so no thread can read a value another one has already replaced.
//       k_mcmc_scatter : blockIdx.y = tensor (k_gather_rows' shape): copy xyz / f_dc / f_rest / rotation rows src -> dst,
//                        write the staged opacity and scale to dst AND src (the pairs of one source store identical bits),
//                        zero the moment rows of dst and src.
//     den is a double sum of up to 1326 terms with the binomials from a host-built table (float loses 2.4e-4 of it at o = 1 -
//     6e-8, N = 51); at most ~5 % of the rows, once per 100 iterations.
//   position noise (lr_mcmc_noise), every iteration: xyz += Sigma xi g(o) scaler, Sigma = R diag(s^2) R^T as preprocess builds it.
//     One thread per Gaussian, 56 B read + 12 B written, HBM-bound.
//   regularisers (lr_mcmc_reg_grad): the gradient of opacity_reg mean(sigmoid(o)) + scale_reg mean(exp(s)) added in place.
#include "common.h"
#include <cmath>
#include <mutex>

namespace lr {

namespace {

constexpr int MC_THREADS = 256;

__global__ void __launch_bounds__(MC_THREADS)
k_mcmc_count(int n, const int* __restrict__ src, int* __restrict__ count)
{
    const int j = blockIdx.x * MC_THREADS + threadIdx.x;
    if (j < n) atomicAdd(&count[src[j]], 1);
}

// table: [MCMC_N_MAX][MCMC_N_MAX] binomials C(a, k) (0 above the diagonal), then MCMC_N_MAX weights (-1)^k / sqrt(k + 1)
__global__ void __launch_bounds__(MC_THREADS)
k_mcmc_compute(int n, const int* __restrict__ src, const int* __restrict__ count, const float* __restrict__ raw_opacity,
               const float* __restrict__ raw_scale, const double* __restrict__ table, float min_opacity, int n_max,
               float4* __restrict__ staged)
{
    const int j = blockIdx.x * MC_THREADS + threadIdx.x;
    if (j >= n) return;
    const int i = src[j];
    const int N = min(count[i] + 1, n_max);
    const float o = fminf(act_opacity(raw_opacity[i]), 1.0f - 0x1p-24f);
    // 1 - (1 - o)^(1/N) without the cancellation of the naive form at small o
    const float o_new = -expm1f(log1pf(-o) / (float)N);
    // den = sum_{m=1..N} sum_{k=0..m-1} C(m-1, k) (-1)^k / sqrt(k+1) o'^(k+1): powers by recurrence, in double
    const double* __restrict__ weight = table + MCMC_N_MAX * MCMC_N_MAX;
    const double od = (double)o_new;
    double den = 0.0;
    for (int m = 1; m <= N; m++) {
        const double* __restrict__ binom = table + (m - 1) * MCMC_N_MAX;
        double pw = od;
        for (int k = 0; k < m; k++) {
            den += binom[k] * weight[k] * pw;
            pw *= od;
        }
    }
    const double ratio = (double)o / den;
    float4 out;
    const float oc = fminf(fmaxf(o_new, min_opacity), 1.0f - 1.1920929e-7f);
    float raw = logf(oc / (1.0f - oc));
    // an opacity clamped from below must read back as alive through the activation every kernel of the library applies
    // (sigmoid(raw) > min_opacity; logit and sigmoid round independently): at most a few ulp of raw
    for (int it = 0; it < 4 && !(act_opacity(raw) > min_opacity); it++) raw = nextafterf(raw, 3.0e38f);
    out.x = raw;
    out.y = logf((float)((double)act_scale(raw_scale[3 * (size_t)i]) * ratio));
    out.z = logf((float)((double)act_scale(raw_scale[3 * (size_t)i + 1]) * ratio));
    out.w = logf((float)((double)act_scale(raw_scale[3 * (size_t)i + 2]) * ratio));
    staged[j] = out;
}

constexpr int MC_MAX_TENSORS = 18;         // six parameters + twelve moments
enum { MC_COPY = 0, MC_STAGED = 1, MC_ZERO = 2 };
struct McTensors {
    float* p[MC_MAX_TENSORS];
    uint32_t row_words[MC_MAX_TENSORS];
    uint8_t mode[MC_MAX_TENSORS];
    uint8_t staged_off[MC_MAX_TENSORS];    // MC_STAGED: first float of the pair's staged record
    int count;
};

__global__ void __launch_bounds__(MC_THREADS)
k_mcmc_scatter(int n, const int* __restrict__ dst, const int* __restrict__ src, const float* __restrict__ staged, McTensors T)
{
    const int t = blockIdx.y;
    const uint32_t w = T.row_words[t];
    const unsigned long long q = (unsigned long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (q >= (unsigned long long)n * w) return;
    const uint32_t j = (uint32_t)(q / w), c = (uint32_t)(q - (unsigned long long)j * w);
    float* __restrict__ p = T.p[t];
    const size_t d = (size_t)dst[j] * w + c, s = (size_t)src[j] * w + c;
    if (T.mode[t] == MC_COPY) p[d] = p[s];
    else {
        const float v = T.mode[t] == MC_STAGED ? staged[4 * (size_t)j + T.staged_off[t] + c] : 0.0f;
        p[d] = v;
        p[s] = v;
    }
}

__global__ void __launch_bounds__(MC_THREADS)
k_mcmc_noise(int P, float* __restrict__ xyz, const float* __restrict__ raw_scale, const float* __restrict__ raw_rotation,
             const float* __restrict__ raw_opacity, const float* __restrict__ noise, float scaler)
{
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= P) return;
    const size_t i3 = 3 * (size_t)i;
    const float4 q = reinterpret_cast<const float4*>(raw_rotation)[i];
    const float nx = noise[i3], ny = noise[i3 + 1], nz = noise[i3 + 2];
    const float sx = act_scale(raw_scale[i3]), sy = act_scale(raw_scale[i3 + 1]), sz = act_scale(raw_scale[i3 + 2]);
    const float o = act_opacity(raw_opacity[i]);
    float px = xyz[i3], py = xyz[i3 + 1], pz = xyz[i3 + 2];
    const float inv = act_quat_inv_norm(q.x, q.y, q.z, q.w);
    const float r = q.x * inv, x = q.y * inv, y = q.z * inv, z = q.w * inv;
    // the rotation preprocess builds (gauss_project.h; c[k] is row k)
    const M3 R = quat_rotation(r, x, y, z);
    const float r00 = R.c[0][0], r01 = R.c[0][1], r02 = R.c[0][2], r10 = R.c[1][0], r11 = R.c[1][1], r12 = R.c[1][2];
    const float r20 = R.c[2][0], r21 = R.c[2][1], r22 = R.c[2][2];
    // Sigma xi = R (s^2 * (R^T xi))
    const float vx = (r00 * nx + r10 * ny + r20 * nz) * (sx * sx);
    const float vy = (r01 * nx + r11 * ny + r21 * nz) * (sy * sy);
    const float vz = (r02 * nx + r12 * ny + r22 * nz) * (sz * sz);
    // the switch that keeps opaque Gaussians still: 1 / (1 + exp(-100 ((1 - o) - 0.995))); exp overflows to inf -> 0
    const float gate = 1.0f / (1.0f + expf(-100.0f * ((1.0f - o) - 0.995f)));
    const float f = gate * scaler;
    px += (r00 * vx + r01 * vy + r02 * vz) * f;
    py += (r10 * vx + r11 * vy + r12 * vz) * f;
    pz += (r20 * vx + r21 * vy + r22 * vz) * f;
    xyz[i3] = px; xyz[i3 + 1] = py; xyz[i3 + 2] = pz;
}

__global__ void __launch_bounds__(MC_THREADS)
k_mcmc_reg_grad(int P, const float* __restrict__ raw_opacity, const float* __restrict__ raw_scale, float w_opacity, float w_scale,
                float* __restrict__ dL_dopacity, float* __restrict__ dL_dscale)
{
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= P) return;
    const size_t i3 = 3 * (size_t)i;
    const float o = act_opacity(raw_opacity[i]);
    dL_dopacity[i] += w_opacity * (o * (1.0f - o));
    dL_dscale[i3] += w_scale * act_scale(raw_scale[i3]);
    dL_dscale[i3 + 1] += w_scale * act_scale(raw_scale[i3 + 1]);
    dL_dscale[i3 + 2] += w_scale * act_scale(raw_scale[i3 + 2]);
}

// C(a, k) for a, k < MCMC_N_MAX (exact in double: C(50, 25) < 2^47) and the signed weights, built once on the host
const double* mcmc_host_table()
{
    static double table[MCMC_TABLE_DOUBLES];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int a = 0; a < MCMC_N_MAX; a++)
            for (int k = 0; k < MCMC_N_MAX; k++)
                table[a * MCMC_N_MAX + k] = k > a ? 0.0 : (k == 0 || k == a) ? 1.0
                                            : table[(a - 1) * MCMC_N_MAX + k - 1] + table[(a - 1) * MCMC_N_MAX + k];
        for (int k = 0; k < MCMC_N_MAX; k++)
            table[MCMC_N_MAX * MCMC_N_MAX + k] = ((k & 1) ? -1.0 : 1.0) / std::sqrt((double)(k + 1));
    });
    return table;
}

struct McLayout { size_t count, staged, table, total; };
McLayout mcmc_layout(int P_rows, int n)
{
    McLayout L; size_t o = 0;
    L.count = o;  o += align_up((size_t)(P_rows > 0 ? P_rows : 1) * 4);
    L.staged = o; o += align_up((size_t)(n > 0 ? n : 1) * 16);
    L.table = o;  o += align_up(MCMC_TABLE_DOUBLES * sizeof(double));
    L.total = o;
    return L;
}

}  // namespace

size_t mcmc_workspace_bytes(int P_rows, int n) { return mcmc_layout(P_rows, n).total; }

hipError_t launch_mcmc_relocate(int n, const int* dst, const int* src, int P_rows, int n_rest, float* const params[6],
                                float* const exp_avg[6], float* const exp_avg_sq[6], float min_opacity, int n_max, char* ws,
                                hipStream_t s)
{
    const McLayout L = mcmc_layout(P_rows, n);
    int* count = reinterpret_cast<int*>(ws + L.count);
    float4* staged = reinterpret_cast<float4*>(ws + L.staged);
    double* table = reinterpret_cast<double*>(ws + L.table);
    hipError_t e = hipMemsetAsync(count, 0, (size_t)P_rows * 4, s);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(table, mcmc_host_table(), MCMC_TABLE_DOUBLES * sizeof(double), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    const dim3 grid((n + MC_THREADS - 1) / MC_THREADS), block(MC_THREADS);
    hipLaunchKernelGGL(k_mcmc_count, grid, block, 0, s, n, src, count);
    hipLaunchKernelGGL(k_mcmc_compute, grid, block, 0, s, n, src, count, params[3], params[4], table, min_opacity, n_max, staged);
    // xyz, f_dc, f_rest, opacity, scaling, rotation: floats per row and what happens to the row
    const uint32_t words[6] = { 3u, 3u, 3u * (uint32_t)n_rest, 1u, 3u, 4u };
    const uint8_t mode[6] = { MC_COPY, MC_COPY, MC_COPY, MC_STAGED, MC_STAGED, MC_COPY };
    const uint8_t off[6] = { 0, 0, 0, 0, 1, 0 };
    McTensors T;
    T.count = 0;
    uint32_t max_words = 0;
    auto add = [&](float* p, uint32_t w, uint8_t m, uint8_t o) {
        if (!p || w == 0) return;
        T.p[T.count] = p; T.row_words[T.count] = w; T.mode[T.count] = m; T.staged_off[T.count] = o;
        T.count++;
        if (w > max_words) max_words = w;
    };
    for (int g = 0; g < 6; g++) add(params[g], words[g], mode[g], off[g]);
    for (int g = 0; g < 6; g++) { add(exp_avg[g], words[g], MC_ZERO, 0); add(exp_avg_sq[g], words[g], MC_ZERO, 0); }
    for (int t = T.count; t < MC_MAX_TENSORS; t++) { T.p[t] = nullptr; T.row_words[t] = 1; T.mode[t] = MC_ZERO; T.staged_off[t] = 0; }
    const unsigned long long total = (unsigned long long)n * max_words;
    hipLaunchKernelGGL(k_mcmc_scatter, dim3((unsigned)((total + MC_THREADS - 1) / MC_THREADS), T.count), block, 0, s, n, dst, src,
                       reinterpret_cast<const float*>(staged), T);
    return hipGetLastError();
}

void launch_mcmc_noise(int P, float* xyz, const float* raw_scale, const float* raw_rotation, const float* raw_opacity,
                       const float* noise, float scaler, hipStream_t s)
{
    hipLaunchKernelGGL(k_mcmc_noise, dim3((P + MC_THREADS - 1) / MC_THREADS), dim3(MC_THREADS), 0, s, P, xyz, raw_scale,
                       raw_rotation, raw_opacity, noise, scaler);
}

void launch_mcmc_reg_grad(int P, const float* raw_opacity, const float* raw_scale, float opacity_reg, float scale_reg,
                          float* dL_dopacity, float* dL_dscale, hipStream_t s)
{
    // the means' 1 / P and 1 / (3 P), formed in double and rounded once
    hipLaunchKernelGGL(k_mcmc_reg_grad, dim3((P + MC_THREADS - 1) / MC_THREADS), dim3(MC_THREADS), 0, s, P, raw_opacity, raw_scale,
                       (float)((double)opacity_reg / P), (float)((double)scale_reg / (3.0 * P)), dL_dopacity, dL_dscale);
}

}  // namespace lr
