// normals.hip -- surface normals from a depth map and the fused normal losses for gfx950 (include/lucid_raster.h, lr_normals_args;
// DESIGN.md 4b-NRM).
//
// The definition is the header's, operation by operation in float32 (this file is compiled with -ffp-contract=off, and hipcc's
// float division and square root are correctly rounded): a numpy float32 restatement gives the same bits.
//   k_depth_normals      : one thread per pixel, five depths in, three planes out.
//   k_depth_normals_bwd  : dL/ddepth from dL/dnormals.
//   k_normal_loss_fwd    : w (1 - n.t) per counted pixel, FWD_ROWS rows of 64 pixels per workgroup, {sum, count} per workgroup
//                          (double, fixed order), then
//   k_normal_loss_final  : one workgroup sums the partials in a fixed order -> {loss, count}.
//   k_normal_loss_bwd    : dL/ddepth of the loss; launched a second time with the two depths swapped for dL/dtarget_depth.
// Both backwards are GATHERS: a normal depends on its pixel's four neighbours, so an output pixel sums the terms of its W, E, N
// and S neighbours' normals.  A workgroup owns 64 x BWD_ROWS output pixels: its threads compute the four terms of every pixel
// of that tile and a one-pixel halo into LDS (the halo's corners are never read), then every output pixel adds its four terms
// from LDS in the fixed order.  No atomics.  The alternative that recomputes the four neighbour normals per output pixel
// straight from the 13-point diamond of depths (no LDS, no barrier, 4x the arithmetic) measured slower: DESIGN.md 4b-NRM.
// A wave covers 64 consecutive pixels of one row: every global load and store is coalesced, every LDS access conflict-free.
#include "common.h"
#include <cmath>

namespace lr {

namespace {

constexpr int NB_X = 64;                   // a wave is one row segment
constexpr int NB_Y = 4;
constexpr int NTHREADS = NB_X * NB_Y;      // 256

struct NCam { float ax, ay, tx, ty; };     // ax = (2 tan_fovx) / W, ay = (2 tan_fovy) / H, tx = tan_fovx, ty = tan_fovy

struct NormalAt {
    bool valid;
    float n0, n1, n2, len;
    float u, v, p, r, gx, gy;              // what the chain back to the depths reads
};

struct Terms { float tE, tW, tS, tN; };    // d / d(depth of the E, W, S, N neighbour)

// The normal of pixel (x, y): the header's operations in the header's order.  Nothing is loaded for a pixel that is not
// interior, so every address is inside the image.
__device__ __forceinline__ NormalAt normal_at(const float* __restrict__ d, int H, int W, int x, int y, NCam c)
{
    NormalAt o;
    o.valid = false;
    o.n0 = o.n1 = o.n2 = 0.f;
    o.len = 1.f;
    o.u = o.v = o.p = o.r = o.gx = o.gy = 0.f;
    if (x < 1 || y < 1 || x > W - 2 || y > H - 2) return o;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    const float dc = d[i], dE = d[i + 1], dW = d[i - 1], dN = d[i - (size_t)W], dS = d[i + (size_t)W];
    o.u = c.ax * ((float)x + 0.5f) - c.tx;
    o.v = c.ay * ((float)y + 0.5f) - c.ty;
    o.gx = dE - dW;
    const float sx = dE + dW;
    o.gy = dS - dN;
    const float sy = dS + dN;
    o.p = c.ax * sx;
    o.r = c.ay * sy;
    const float a = o.r * o.gx, b = o.p * o.gy;
    const float c2 = -((b * o.v + a * o.u) + o.p * o.r);
    const float m2 = (a * a + b * b) + c2 * c2;
    if (!(dc > 0.f && dE > 0.f && dW > 0.f && dN > 0.f && dS > 0.f && m2 > 0.f && m2 < INFINITY)) return o;
    o.len = sqrtf(m2);
    o.n0 = a / o.len;
    o.n1 = b / o.len;
    o.n2 = c2 / o.len;
    o.valid = true;
    return o;
}

// from G = dL/dc to the four neighbour depths
__device__ __forceinline__ Terms chain(const NormalAt& o, NCam c, float G0, float G1, float G2)
{
    const float A = G0 - o.u * G2, B = G1 - o.v * G2;
    const float dgx = o.r * A, dgy = o.p * B;
    const float dsx = c.ax * (o.gy * B - o.r * G2);
    const float dsy = c.ay * (o.gx * A - o.p * G2);
    Terms t;
    t.tE = dgx + dsx;
    t.tW = dsx - dgx;
    t.tS = dgy + dsy;
    t.tN = dsy - dgy;
    return t;
}

struct Plane { int H, W; NCam cam; };

__device__ __forceinline__ bool block_pixel(const Plane& g, int blocks_x, int& x, int& y)
{
    const int bx = (int)(blockIdx.x % (unsigned)blocks_x), by = (int)(blockIdx.x / (unsigned)blocks_x);
    x = bx * NB_X + (int)(threadIdx.x & (NB_X - 1));
    y = by * NB_Y + (int)(threadIdx.x / NB_X);
    return x < g.W && y < g.H;
}

__global__ void __launch_bounds__(NTHREADS)
k_depth_normals(Plane g, int blocks_x, const float* __restrict__ depth, float* __restrict__ out)
{
    int x, y;
    if (!block_pixel(g, blocks_x, x, y)) return;
    const NormalAt o = normal_at(depth, g.H, g.W, x, y, g.cam);
    const size_t n = (size_t)g.H * (size_t)g.W, i = (size_t)y * (size_t)g.W + (size_t)x;
    out[i] = o.n0;
    out[i + n] = o.n1;
    out[i + 2 * n] = o.n2;
}

// the terms of pixel (x, y)'s normal under the upstream Gn [3,H,W]
__device__ __forceinline__ Terms vjp_terms(const Plane& g, const float* __restrict__ depth, const float* __restrict__ Gn, int x, int y)
{
    const Terms z = { 0.f, 0.f, 0.f, 0.f };
    const NormalAt o = normal_at(depth, g.H, g.W, x, y, g.cam);
    if (!o.valid) return z;
    const size_t n = (size_t)g.H * (size_t)g.W, i = (size_t)y * (size_t)g.W + (size_t)x;
    const float g0 = Gn[i], g1 = Gn[i + n], g2 = Gn[i + 2 * n];
    const float dn = (o.n0 * g0 + o.n1 * g1) + o.n2 * g2;
    return chain(o, g.cam, (g0 - o.n0 * dn) / o.len, (g1 - o.n1 * dn) / o.len, (g2 - o.n2 * dn) / o.len);
}

// The gather of a 64 x BWD_ROWS tile: terms_of(x, y) is the Terms of pixel (x, y), zero where it does not count.
constexpr int BWD_ROWS = 8;                // 66 x 10 pixels computed for 64 x 8 written (1.29x; 4 rows: 1.55x, measured slower)
constexpr int TW = NB_X + 2, TH = BWD_ROWS + 2;
struct Tile { float E[TH][TW], W[TH][TW], S[TH][TW], N[TH][TW]; };

template <class F>
__device__ __forceinline__ void gather_tile(const Plane& g, int blocks_x, Tile& s, float* __restrict__ grad, F terms_of)
{
    const int bx = (int)(blockIdx.x % (unsigned)blocks_x), by = (int)(blockIdx.x / (unsigned)blocks_x);
    const int x0 = bx * NB_X - 1, y0 = by * BWD_ROWS - 1;
    for (int e = (int)threadIdx.x; e < TW * TH; e += NTHREADS) {
        const int ly = e / TW, lx = e - ly * TW;
        const bool corner = (lx == 0 || lx == TW - 1) && (ly == 0 || ly == TH - 1);
        Terms t = { 0.f, 0.f, 0.f, 0.f };
        if (!corner) t = terms_of(x0 + lx, y0 + ly);
        s.E[ly][lx] = t.tE; s.W[ly][lx] = t.tW; s.S[ly][lx] = t.tS; s.N[ly][lx] = t.tN;
    }
    lds_barrier();
    const int lx = (int)(threadIdx.x & (NB_X - 1)) + 1, x = x0 + lx;
    if (x >= g.W) return;
    for (int ly = (int)(threadIdx.x / NB_X) + 1; ly <= BWD_ROWS; ly += NB_Y) {
        const int y = y0 + ly;
        if (y < g.H)
            grad[(size_t)y * (size_t)g.W + (size_t)x] = ((s.E[ly][lx - 1] + s.W[ly][lx + 1]) + s.S[ly - 1][lx]) + s.N[ly + 1][lx];
    }
}

__global__ void __launch_bounds__(NTHREADS)
k_depth_normals_bwd(Plane g, int blocks_x, const float* __restrict__ depth, const float* __restrict__ Gn, float* __restrict__ grad)
{
    __shared__ Tile s;
    gather_tile(g, blocks_x, s, grad, [&](int x, int y) { return vjp_terms(g, depth, Gn, x, y); });
}

// ---- the loss ----
struct LossIn {
    const float* depth;
    const float* target_normals;           // [3,H,W], or
    const float* target_depth;             // [H,W]
    const float* pixel_weight;             // [H,W] or NULL
};

// Does pixel (x, y) count?  Then o is its normal, t its unit target, dot = n.t, w its weight.
template <bool CONSIST>
__device__ __forceinline__ bool loss_pixel(const Plane& g, const LossIn& in, int x, int y, NormalAt& o, float& t0, float& t1,
                                           float& t2, float& dot, float& w)
{
    o = normal_at(in.depth, g.H, g.W, x, y, g.cam);
    if (!o.valid) return false;
    const size_t n = (size_t)g.H * (size_t)g.W, i = (size_t)y * (size_t)g.W + (size_t)x;
    w = 1.f;
    if (in.pixel_weight != nullptr) {
        w = in.pixel_weight[i];
        if (!(w > 0.f)) return false;
    }
    if (CONSIST) {
        const NormalAt t = normal_at(in.target_depth, g.H, g.W, x, y, g.cam);
        if (!t.valid) return false;
        t0 = t.n0; t1 = t.n1; t2 = t.n2;
    } else {
        const float a0 = in.target_normals[i], a1 = in.target_normals[i + n], a2 = in.target_normals[i + 2 * n];
        const float tt = (a0 * a0 + a1 * a1) + a2 * a2;
        if (!(tt > 0.f && tt < INFINITY)) return false;
        const float tl = sqrtf(tt);
        t0 = a0 / tl; t1 = a1 / tl; t2 = a2 / tl;
    }
    dot = (o.n0 * t0 + o.n1 * t1) + o.n2 * t2;
    return true;
}

constexpr int FWD_ROWS = 16;               // rows per workgroup of the loss forward: 4 pixels per thread, a quarter of the partials

template <bool CONSIST>
__global__ void __launch_bounds__(NTHREADS)
k_normal_loss_fwd(Plane g, int blocks_x, LossIn in, double2* __restrict__ partials)
{
    __shared__ double s_sum[NTHREADS / 64];
    __shared__ int s_cnt[NTHREADS / 64];
    const int bx = (int)(blockIdx.x % (unsigned)blocks_x), by = (int)(blockIdx.x / (unsigned)blocks_x);
    const int x = bx * NB_X + (int)(threadIdx.x & (NB_X - 1));
    double v = 0.0;
    int counted = 0;
#pragma unroll
    for (int i = 0; i < FWD_ROWS / NB_Y; i++) {          // rows ty, ty + 4, ...: summed in this order
        const int y = by * FWD_ROWS + i * NB_Y + (int)(threadIdx.x / NB_X);
        NormalAt o;
        float t0, t1, t2, dot, w;
        if (x < g.W && y < g.H && loss_pixel<CONSIST>(g, in, x, y, o, t0, t1, t2, dot, w)) {
            v += (double)(w * (1.0f - dot));
            counted += 1;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v += __shfl_xor(v, off);
        counted += __shfl_xor(counted, off);
    }
    const int wv = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_sum[wv] = v; s_cnt[wv] = counted; }
    lds_barrier();
    if (threadIdx.x == 0)
        partials[blockIdx.x] = make_double2((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]),
                                            (double)((s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3])));
}

__global__ void __launch_bounds__(NTHREADS)
k_normal_loss_final(int n_blocks, double n_elems, float weight, const double2* __restrict__ partials, float* __restrict__ out)
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

template <bool CONSIST>
__device__ __forceinline__ Terms loss_terms(const Plane& g, const LossIn& in, int x, int y, float k)
{
    const Terms z = { 0.f, 0.f, 0.f, 0.f };
    NormalAt o;
    float t0, t1, t2, dot, w;
    if (!loss_pixel<CONSIST>(g, in, x, y, o, t0, t1, t2, dot, w)) return z;
    const float q = k * w;
    const float kk = q / o.len;
    return chain(o, g.cam, -(kk * (t0 - o.n0 * dot)), -(kk * (t1 - o.n1 * dot)), -(kk * (t2 - o.n2 * dot)));
}

template <bool CONSIST>
__global__ void __launch_bounds__(NTHREADS)
k_normal_loss_bwd(Plane g, int blocks_x, LossIn in, float weight, const float* __restrict__ upstream, float* __restrict__ grad)
{
    __shared__ Tile s;
    const float up = upstream != nullptr ? upstream[0] : 1.0f;
    const float k = (up * weight) / (float)(g.H * g.W);
    gather_tile(g, blocks_x, s, grad, [&](int x, int y) { return loss_terms<CONSIST>(g, in, x, y, k); });
}

// ---- the two geometry terms of the multi-view step (lr_views_accumulate with distortion_weight / normal_consistency_weight) ----
// k_geom_terms: per pixel the distortion D and the consistency term 1 - N.n between the rendered normal map N and the depth
// normals n (what k_depth_normals wrote: an invalid pixel is (0,0,0) and adds nothing), {sum D, sum (1 - N.n)} per workgroup in
// double and a fixed order, the shape of k_normal_loss_fwd.  With kn = weight / (H W) != 0 it also leaves the two upstream images
// of the term's backward: dL/dN = -kn n IN PLACE of n (exact zeros on the invalid pixels) and dL/dn = -kn N in gn_up (what
// k_depth_normals_bwd takes as Gn; it skips the invalid pixels itself).
__global__ void __launch_bounds__(NTHREADS)
k_geom_terms(int H, int W, int blocks_x, const float* __restrict__ dist, const float* __restrict__ nmap, float* __restrict__ n_io,
             float* __restrict__ gn_up, float kn, double2* __restrict__ partials)
{
    __shared__ double s_d[NTHREADS / 64], s_c[NTHREADS / 64];
    const int bx = (int)(blockIdx.x % (unsigned)blocks_x), by = (int)(blockIdx.x / (unsigned)blocks_x);
    const int x = bx * NB_X + (int)(threadIdx.x & (NB_X - 1));
    const size_t n = (size_t)H * (size_t)W;
    double vd = 0.0, vc = 0.0;
#pragma unroll
    for (int r = 0; r < FWD_ROWS / NB_Y; r++) {          // rows ty, ty + 4, ...: summed in this order
        const int y = by * FWD_ROWS + r * NB_Y + (int)(threadIdx.x / NB_X);
        if (x < W && y < H) {
            const size_t i = (size_t)y * (size_t)W + (size_t)x;
            vd += (double)dist[i];
            const float n0 = n_io[i], n1 = n_io[i + n], n2 = n_io[i + 2 * n];
            const float N0 = nmap[i], N1 = nmap[i + n], N2 = nmap[i + 2 * n];
            const bool valid = n0 != 0.f || n1 != 0.f || n2 != 0.f;
            if (valid) vc += (double)(1.0f - ((N0 * n0 + N1 * n1) + N2 * n2));
            if (kn != 0.f) {
                n_io[i] = valid ? -(kn * n0) : 0.f; n_io[i + n] = valid ? -(kn * n1) : 0.f; n_io[i + 2 * n] = valid ? -(kn * n2) : 0.f;
                gn_up[i] = -(kn * N0); gn_up[i + n] = -(kn * N1); gn_up[i + 2 * n] = -(kn * N2);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        vd += __shfl_xor(vd, off);
        vc += __shfl_xor(vc, off);
    }
    const int wv = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_d[wv] = vd; s_c[wv] = vc; }
    lds_barrier();
    if (threadIdx.x == 0)
        partials[blockIdx.x] = make_double2((s_d[0] + s_d[1]) + (s_d[2] + s_d[3]), (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]));
}

// one workgroup: the partials in a fixed order -> the view's seven-column row {loss, l1, ssim, depth term, alpha_hole, distortion,
// normal_consistency}: out[5] = mean(D), out[6] = sum (1 - N.n) / (H W), out[0] += wd out[5] + wn out[6]; the columns of a term
// the step does not have are set to 0.  Behind every other term of the row on the view's stream.
__global__ void __launch_bounds__(NTHREADS)
k_geom_terms_final(int n_blocks, double n_elems, float wd, float wn, int row_has_depth, int row_has_alpha,
                   const double2* __restrict__ partials, float* __restrict__ out)
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
        const float d = (float)(s_a[0] / n_elems), c = (float)(s_b[0] / n_elems);
        out[0] = (out[0] + wd * d) + wn * c;
        if (!row_has_depth) out[3] = 0.f;
        if (!row_has_alpha) out[4] = 0.f;
        out[5] = d;
        out[6] = c;
    }
}

// dst += src, elementwise
__global__ void __launch_bounds__(256) k_plane_add(long long n, float* __restrict__ dst, const float* __restrict__ src)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

Plane plane_of(const lr_normals_args& a)
{
    Plane g;
    g.H = a.height;
    g.W = a.width;
    g.cam.ax = (2.0f * a.tan_fovx) / (float)a.width;
    g.cam.ay = (2.0f * a.tan_fovy) / (float)a.height;
    g.cam.tx = a.tan_fovx;
    g.cam.ty = a.tan_fovy;
    return g;
}

int blocks_x_of(int W) { return (W + NB_X - 1) / NB_X; }
int blocks_of(int H, int W, int rows) { return blocks_x_of(W) * ((H + rows - 1) / rows); }     // <= H*W < 2^31

}  // namespace

size_t normals_workspace_bytes(int H, int W) { return align_up((size_t)blocks_of(H, W, FWD_ROWS) * sizeof(double2)); }

void launch_depth_normals(const lr_normals_args& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_depth_normals, dim3(blocks_of(a.height, a.width, NB_Y)), dim3(NTHREADS), 0, s, plane_of(a),
                       blocks_x_of(a.width), a.depth, a.out_normals);
}

void launch_depth_normals_backward(const lr_normals_args& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_depth_normals_bwd, dim3(blocks_of(a.height, a.width, BWD_ROWS)), dim3(NTHREADS), 0, s, plane_of(a),
                       blocks_x_of(a.width), a.depth, a.dL_dnormals, a.dL_ddepth);
}

void launch_normal_loss_forward(const lr_normals_args& a, hipStream_t s)
{
    const int blocks = blocks_of(a.height, a.width, FWD_ROWS), bx = blocks_x_of(a.width);
    const LossIn in = { a.depth, a.target_normals, a.target_depth, a.pixel_weight };
    double2* partials = static_cast<double2*>(a.workspace);
    if (a.target_depth != nullptr)
        hipLaunchKernelGGL(k_normal_loss_fwd<true>, dim3(blocks), dim3(NTHREADS), 0, s, plane_of(a), bx, in, partials);
    else
        hipLaunchKernelGGL(k_normal_loss_fwd<false>, dim3(blocks), dim3(NTHREADS), 0, s, plane_of(a), bx, in, partials);
    hipLaunchKernelGGL(k_normal_loss_final, dim3(1), dim3(NTHREADS), 0, s, blocks, (double)a.height * (double)a.width, a.weight,
                       partials, a.out);
}

void launch_normal_loss_backward(const lr_normals_args& a, hipStream_t s)
{
    const int blocks = blocks_of(a.height, a.width, BWD_ROWS), bx = blocks_x_of(a.width);
    const LossIn in = { a.depth, a.target_normals, a.target_depth, a.pixel_weight };
    if (a.target_depth == nullptr) {
        hipLaunchKernelGGL(k_normal_loss_bwd<false>, dim3(blocks), dim3(NTHREADS), 0, s, plane_of(a), bx, in, a.weight, a.upstream,
                           a.dL_ddepth);
        return;
    }
    hipLaunchKernelGGL(k_normal_loss_bwd<true>, dim3(blocks), dim3(NTHREADS), 0, s, plane_of(a), bx, in, a.weight, a.upstream,
                       a.dL_ddepth);
    if (a.dL_dtarget_depth != nullptr) {                 // the same term with the roles of the two depths swapped
        const LossIn swapped = { a.target_depth, nullptr, a.depth, a.pixel_weight };
        hipLaunchKernelGGL(k_normal_loss_bwd<true>, dim3(blocks), dim3(NTHREADS), 0, s, plane_of(a), bx, swapped, a.weight,
                           a.upstream, a.dL_dtarget_depth);
    }
}

size_t geom_terms_workspace_bytes(int H, int W) { return align_up((size_t)blocks_of(H, W, FWD_ROWS) * sizeof(double2)); }

void launch_geom_terms(const GeomTerms& t, hipStream_t s)
{
    const int blocks = blocks_of(t.H, t.W, FWD_ROWS);
    double2* partials = reinterpret_cast<double2*>(t.ws);
    const float kn = t.normal_weight / (float)(t.H * t.W);
    hipLaunchKernelGGL(k_geom_terms, dim3(blocks), dim3(NTHREADS), 0, s, t.H, t.W, blocks_x_of(t.W), t.distortion, t.normals, t.n_io,
                       t.gn_up, kn, partials);
    hipLaunchKernelGGL(k_geom_terms_final, dim3(1), dim3(NTHREADS), 0, s, blocks, (double)t.H * (double)t.W, t.distortion_weight,
                       t.normal_weight, t.row_has_depth ? 1 : 0, t.row_has_alpha ? 1 : 0, partials, t.out_row);
}

void launch_plane_add(long long n, float* dst, const float* src, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_plane_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, dst, src);
}

}  // namespace lr
