// dream.hip -- what generate_pcd does between its networks and the append of the new points (R/luciddreamer.py:424-493) for
// gfx950: the scale of the new depth map against the cloud, the depth offsets along the hole's border, their interpolation into
// every hole pixel, and the lift of the corrected depth.  Semantics, operation by operation: include/lucid_raster.h (lr_dream_*,
// lr_scatter_interpolate); tests/dream_ref.py restates them in numpy.
//
//   k_scale_partial / k_scale_final : Spp, Spq, Sqq and the pair count over the valid points.  One term per thread, a fixed
//               tree over the workgroup's 256 terms in LDS, then the workgroup partials in index order by one lane (staged
//               through LDS 64 at a time).  No float atomics: two runs give the same bits.
//   k_correspond : per border correspondence the exact projected coordinates (project_point, shared with reproject.hip) and the
//               depth offset between the cloud point's foot on the camera ray and the new depth; the four zero corners last.
//   k_interp  : the hot kernel.  One thread per pixel; a workgroup without a hole pixel leaves before the loop.  Samples are
//               staged through LDS in tiles of LR_SCATTER_TILE (three float64 planes, 6 KB); every lane reads the same sample (a
//               broadcast, no bank conflict) and accumulates sequentially in the sample index: 9 + 2 float64 accumulators, about
//               25 float64 operations and one correctly rounded division per pixel and sample.  A NaN sample is skipped by a
//               wave-uniform branch.
//   k_dream_lift : float32(s * liftw(x, y, D + nd)) per pixel.
// All arithmetic is float64 in a fixed order, one IEEE operation each (the TU is compiled with -ffp-contract=off).
#include "common.h"
#include "lucid_raster.h"
#include "project_point.h"

namespace lr {

namespace {

constexpr int DT = DREAM_BLOCK;
static_assert(DT == 256 && LR_SCATTER_TILE == DT, "the tree and the tile loads are written for 256 threads");

struct LiftMats { double Kinv[9], Rinv[9], t[3]; };

struct Partial { double pp, pq, qq; long long n; };

__device__ __forceinline__ void liftw(const LiftMats& m, int x, int y, double d, double w[3])
{
    const double xd = (double)x * d, yd = (double)y * d;
    const double c0 = row3(m.Kinv, xd, yd, d), c1 = row3(m.Kinv + 3, xd, yd, d), c2 = row3(m.Kinv + 6, xd, yd, d);
    w[0] = row3(m.Rinv, c0, c1, c2) - m.t[0];
    w[1] = row3(m.Rinv + 3, c0, c1, c2) - m.t[1];
    w[2] = row3(m.Rinv + 6, c0, c1, c2) - m.t[2];
}

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ bool finite3(const double* a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }

// ---- scale sums ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT) k_scale_partial(LiftMats m, const float* __restrict__ pts, long long ps, long long cs,
                                                      const uint8_t* __restrict__ valid, const int* __restrict__ pix, int N, int W,
                                                      int H, const float* __restrict__ depth, Partial* __restrict__ partial)
{
    __shared__ double s_pp[DT], s_pq[DT], s_qq[DT];
    __shared__ int s_n[DT];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * DT + tid;
    double pp = 0.0, pq = 0.0, qq = 0.0;
    int n = 0;
    if (i < N && valid[i]) {
        const int p = pix[i];
        if (p >= 0 && p < W * H) {                            // a pixel outside the image (not lr_reproject's) is left out
            const int y = p / W, x = p - y * W;
            double q[3];
            liftw(m, x, y, (double)depth[p], q);
            if (finite3(q)) {
                const double P[3] = { (double)pts[(size_t)i * ps], (double)pts[(size_t)i * ps + cs],
                                      (double)pts[(size_t)i * ps + 2 * cs] };
                pp = dot3(P, P);
                pq = dot3(P, q);
                qq = dot3(q, q);
                n = 1;
            }
        }
    }
    s_pp[tid] = pp;
    s_pq[tid] = pq;
    s_qq[tid] = qq;
    s_n[tid] = n;
    for (int st = DT / 2; st > 0; st >>= 1) {
        __syncthreads();
        if (tid < st) {
            s_pp[tid] = s_pp[tid] + s_pp[tid + st];
            s_pq[tid] = s_pq[tid] + s_pq[tid + st];
            s_qq[tid] = s_qq[tid] + s_qq[tid + st];
            s_n[tid] = s_n[tid] + s_n[tid + st];
        }
    }
    if (tid == 0) {
        Partial r;
        r.pp = s_pp[0];
        r.pq = s_pq[0];
        r.qq = s_qq[0];
        r.n = s_n[0];
        partial[blockIdx.x] = r;
    }
}

// one wave: 64 partials at a time into LDS, lane 0 adds them in index order
__global__ void __launch_bounds__(64) k_scale_final(const Partial* __restrict__ partial, int nb, double* __restrict__ out_sums,
                                                    long long* __restrict__ out_count)
{
    __shared__ Partial s_p[64];
    const int tid = threadIdx.x;
    double pp = 0.0, pq = 0.0, qq = 0.0;
    long long n = 0;
    for (int base = 0; base < nb; base += 64) {
        __syncthreads();
        if (base + tid < nb) s_p[tid] = partial[base + tid];
        __syncthreads();
        if (tid == 0) {
            const int m = nb - base < 64 ? nb - base : 64;
            for (int k = 0; k < m; k++) {
                pp = pp + s_p[k].pp;
                pq = pq + s_p[k].pq;
                qq = qq + s_p[k].qq;
                n += s_p[k].n;
            }
        }
    }
    if (tid == 0) {
        out_sums[0] = pp;
        out_sums[1] = pq;
        out_sums[2] = qq;
        out_count[0] = n;
    }
}

// ---- correspondences -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT) k_correspond(Cameras cam, LiftMats m, double s, const float* __restrict__ pts, long long ps,
                                                   long long cs, int N, const int* __restrict__ pix,
                                                   const float* __restrict__ depth, int W, int H, const int* __restrict__ corr,
                                                   int M, double* __restrict__ su, double* __restrict__ sv,
                                                   double* __restrict__ sval)
{
    const int j = blockIdx.x * DT + threadIdx.x;
    if (j >= M + 4) return;
    if (j >= M) {                                             // (0,0), (0,H-1), (W-1,0), (W-1,H-1), value 0
        const int k = j - M;
        su[j] = (k & 2) ? (double)(W - 1) : 0.0;
        sv[j] = (k & 1) ? (double)(H - 1) : 0.0;
        sval[j] = 0.0;
        return;
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int i = corr[j];
    if (i < 0 || i >= N) {                                    // not an index of this cloud: skipped downstream
        su[j] = nan;
        sv[j] = nan;
        sval[j] = nan;
        return;
    }
    const Projected r = project_point(cam, 0, pts, ps, cs, i, W, H);
    su[j] = r.u;
    sv[j] = r.v;
    double value = nan;
    const int p = pix[i];
    if (p >= 0 && p < W * H) {
        const int y = p / W, x = p - y * W;
        double w[3], c[3], a[3], pp[3], mm[3];
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] = 0.0;
        liftw(m, x, y, (double)depth[p], w);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double o = -m.t[k];
            c[k] = s * w[k];
            a[k] = c[k] - o;
            pp[k] = (double)pts[(size_t)i * ps + k * cs] - o;
        }
        const double pa = dot3(pp, a), aa = dot3(a, a);
        const double t = pa / aa;
#pragma unroll
        for (int k = 0; k < 3; k++) mm[k] = -m.t[k] + a[k] * t;
        const double zm = row3(cam.R[0] + 6, mm[0], mm[1], mm[2]) + cam.T[0][2];
        const double zc = row3(cam.R[0] + 6, c[0], c[1], c[2]) + cam.T[0][2];
        value = zm - zc;
        if (aa == 0.0 || !isfinite(value)) value = nan;
    }
    sval[j] = value;
}

// ---- scattered interpolation: moving least squares, affine, inverse-distance weights -------------------------------------------
__global__ void __launch_bounds__(DT) k_interp(const double* __restrict__ su, const double* __restrict__ sv,
                                               const double* __restrict__ sval, int M, int W, int H,
                                               const uint8_t* __restrict__ where, float* __restrict__ out)
{
    __shared__ double s_u[DT], s_v[DT], s_val[DT];
    const int HW = W * H;
    const int tid = threadIdx.x;
    const int p = blockIdx.x * DT + tid;
    const bool live = p < HW;
    const bool query = live && where[p] == 0;
    if (live && !query) out[p] = 0.f;
    if (!__syncthreads_or(query ? 1 : 0)) return;             // a workgroup without a hole pixel
    const int yi = live ? p / W : 0, xi = live ? p - yi * W : 0;
    const double x = (double)xi, y = (double)yi;
    double S00 = 0.0, S01 = 0.0, S02 = 0.0, S11 = 0.0, S12 = 0.0, S22 = 0.0, B0 = 0.0, B1 = 0.0, B2 = 0.0;
    double vmin = __longlong_as_double(0x7ff0000000000000ll), vmax = -vmin;
    int used = 0;
    for (int base = 0; base < M; base += DT) {
        const int n = M - base < DT ? M - base : DT;
        __syncthreads();                                      // the previous tile has been read
        if (tid < n) {
            s_u[tid] = su[base + tid];
            s_v[tid] = sv[base + tid];
            s_val[tid] = sval[base + tid];
        }
        __syncthreads();
        if (query) {
            for (int t = 0; t < n; t++) {
                const double val = s_val[t];
                if (val != val) continue;                     // NaN: the same for every lane
                const double dx = s_u[t] - x, dy = s_v[t] - y;
                const double d2 = (dx * dx + dy * dy) + 1e-12;
                const double w = 1.0 / (d2 * d2);
                const double wx = w * dx, wy = w * dy, wv = w * val;
                S00 = S00 + w;
                S01 = S01 + wx;
                S02 = S02 + wy;
                S11 = S11 + wx * dx;
                S12 = S12 + wx * dy;
                S22 = S22 + wy * dy;
                B0 = B0 + wv;
                B1 = B1 + wv * dx;
                B2 = B2 + wv * dy;
                vmin = val < vmin ? val : vmin;
                vmax = val > vmax ? val : vmax;
                used++;
            }
        }
    }
    if (!query) return;
    float res = 0.f;
    if (used) {
        const double C0 = S11 * S22 - S12 * S12;
        const double C1 = S02 * S12 - S01 * S22;
        const double C2 = S01 * S12 - S02 * S11;
        const double det = (S00 * C0 + S01 * C1) + S02 * C2;
        const double num = (B0 * C0 + B1 * C1) + B2 * C2;
        const double thr = 1e-12 * ((S00 * S11) * S22);
        double r = det > thr ? num / det : B0 / S00;
        r = r > vmin ? r : vmin;                              // max(r, vmin); a NaN r takes vmin
        r = r < vmax ? r : vmax;
        res = (float)r;
    }
    out[p] = res;
}

// ---- compensated lift ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT) k_dream_lift(LiftMats m, double s, int W, int H, const float* __restrict__ depth,
                                                   const float* __restrict__ nd, float* __restrict__ out)
{
    const int HW = W * H;
    const int p = blockIdx.x * DT + threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    const double dd = (double)depth[p] + (double)nd[p];
    double w[3];
    liftw(m, x, y, dd, w);
    out[p] = (float)(s * w[0]);
    out[(size_t)HW + p] = (float)(s * w[1]);
    out[2 * (size_t)HW + p] = (float)(s * w[2]);
}

inline LiftMats lift_mats(const DreamLaunch& a)
{
    LiftMats m;
    for (int k = 0; k < 9; k++) { m.Kinv[k] = a.Kinv[k]; m.Rinv[k] = a.Rinv[k]; }
    for (int k = 0; k < 3; k++) m.t[k] = a.RinvT[k];
    return m;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + DT - 1) / DT); }

}  // namespace

size_t dream_workspace_bytes(long long n_points)
{
    const size_t nb = (size_t)((n_points + DT - 1) / DT);
    return (((nb ? nb : 1) * sizeof(Partial)) + 255) & ~(size_t)255;
}

hipError_t launch_dream_scale_sums(const DreamLaunch& a, hipStream_t s)
{
    Partial* partial = static_cast<Partial*>(a.workspace);
    const unsigned nb = blocks_of(a.n_points);
    if (nb > 0)
        k_scale_partial<<<nb, DT, 0, s>>>(lift_mats(a), a.points, a.point_stride, a.coord_stride, a.valid, a.pix, a.n_points,
                                          a.width, a.height, a.depth, partial);
    k_scale_final<<<1, 64, 0, s>>>(partial, (int)nb, a.out_sums, a.out_count);
    return hipGetLastError();
}

hipError_t launch_dream_correspond(const DreamLaunch& a, hipStream_t s)
{
    Cameras cam;
    for (int k = 0; k < 9; k++) cam.K[k] = a.K[k];
    for (int f = 0; f < REPROJECT_FRAMES_PER_LAUNCH; f++) {
        for (int k = 0; k < 9; k++) cam.R[f][k] = a.R[k];
        for (int k = 0; k < 3; k++) cam.T[f][k] = a.T[k];
    }
    k_correspond<<<blocks_of((long long)a.n_corr + 4), DT, 0, s>>>(cam, lift_mats(a), a.scale, a.points, a.point_stride,
                                                                   a.coord_stride, a.n_points, a.pix, a.depth, a.width, a.height,
                                                                   a.corr, a.n_corr, a.out_su, a.out_sv, a.out_sval);
    return hipGetLastError();
}

hipError_t launch_scatter_interpolate(long long n_samples, const double* su, const double* sv, const double* sval, int height,
                                      int width, const uint8_t* where, float* out, hipStream_t s)
{
    k_interp<<<blocks_of((long long)height * width), DT, 0, s>>>(su, sv, sval, (int)n_samples, width, height, where, out);
    return hipGetLastError();
}

hipError_t launch_dream_lift(const DreamLaunch& a, hipStream_t s)
{
    k_dream_lift<<<blocks_of((long long)a.height * a.width), DT, 0, s>>>(lift_mats(a), a.scale, a.width, a.height, a.depth,
                                                                         a.new_depth, a.out_points);
    return hipGetLastError();
}

}  // namespace lr
