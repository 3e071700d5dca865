// reproject.hip -- the point-cloud reprojection of LucidDreamer's generate_pcd (R/luciddreamer.py:382-413 "Dreaming",
// :516-570 "Aligning") for gfx950: warped frames, hit / hole masks, and the lift of a depth map back into the world.
//
// The reference projects the whole accumulated cloud into every new pose on the host, interpolates an image with
// scipy.interpolate.griddata (a Delaunay triangulation of every projected point) and forms the hole mask with a 9x9 maximum
// and an 11x11 minimum filter.  Here the frames of one cloud are formed on the device, F frames in the same launches
// (frame on grid.y):
//   k_project : p = R x + T, q = K p in float64, validity, rounded pixel, atomicMin of the float32 depth's bits per pixel.
//   k_splat   : the image (our own definition, see the header): a z-tested bilinear splat in fixed point, 64-bit integer
//               atomic adds of weight * colour and weight into the up to four neighbours of every valid point.
//   k_window  : dilation (9x9 maximum of the hit plane) and erosion (11x11 minimum of the dilated plane), separable over an LDS
//               tile with its halo.  Windows are clamped to the image (= scipy's default `reflect` border for max / min).
//   k_resolve : window fill of unhit pixels, normalisation, mask, border (the reference's mask_hf), uint8 packing, depth.
//   k_lift    : inv(R) (inv(K) (x d, y d, d)) - inv(R) T per pixel in float64.
// All projection arithmetic is float64 in a fixed order, ((a0 x + a1 y) + a2 z) + t, one IEEE operation each (the TU is
// compiled with -ffp-contract=off), so a numpy restatement gives the same bits (tests/reproject_ref.py).  Everything that
// depends on arrival order is an integer atomic: two runs give the same bits.
//
// Atomic traffic: a valid point issues one 4-byte atomicMin and at most 4 x 4 8-byte adds (fewer when a
// weight rounds to zero: a point on a pixel centre issues 4).  Clouds lifted from pixel grids put neighbouring points on
// neighbouring pixels, so a wave's adds spread over rows of 32-byte pixel records.  The opposite case, a whole wave in one
// bilinear cell (a far, dense part of the cloud; test case c), is summed across the wave first and issued by one lane.
#include "common.h"
#include "lucid_raster.h"
#include "project_point.h"        // Cameras, Projected, row3, project_point (shared with dream.hip)

namespace lr {

namespace {

constexpr int RT = 256;                         // threads per workgroup of the per-point and per-pixel kernels
constexpr uint32_t NO_HIT = 0xFFFFFFFFu;        // zmin bits of a pixel no point rounded to (the plane is memset to 0xFF)
constexpr int DIL_R = 4, ERO_R = 5;             // 9x9 maximum, 11x11 minimum

// ---- project: validity, rounded pixel, zmin ----------------------------------------------------------------------------------
// grid (ceil(N / RT), frames of this launch).  valid / pix are given only with one frame.
__global__ void __launch_bounds__(RT) k_project(Cameras cam, const float* __restrict__ pts, long long ps, long long cs, int N,
                                                int W, int H, uint32_t* __restrict__ zmin, uint8_t* __restrict__ out_valid,
                                                int* __restrict__ out_pix)
{
    const int i = blockIdx.x * RT + threadIdx.x;
    const int f = blockIdx.y;
    const bool live = i < N;
    Projected p;
    p.valid = false;
    p.iu = p.iv = 0;
    p.z = 0.f;
    if (live) p = project_point(cam, f, pts, ps, cs, i, W, H);
    const int pix = p.iv * W + p.iu;
    if (live && out_valid) out_valid[i] = p.valid ? 1 : 0;
    if (live && out_pix) out_pix[i] = p.valid ? pix : -1;
    // z > 0: the order of the bits is the order of the values.  A wave whose valid lanes all share one pixel sends one atomic.
    uint32_t zb = p.valid ? __float_as_uint(p.z) : NO_HIT;
    const unsigned long long act = __ballot(p.valid);
    if (act == 0ull) return;
    const int first = __ffsll((long long)act) - 1;
    const int pix0 = __shfl(pix, first);
    uint32_t* plane = zmin + (size_t)f * ((size_t)W * H);
    if (__ballot(p.valid && pix == pix0) == act) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)zb, off);
            zb = o < zb ? o : zb;
        }
        if ((int)__lane_id() == first) atomicMin(&plane[pix0], zb);
    } else if (p.valid) {
        atomicMin(&plane[pix], zb);
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// ---- splat -------------------------------------------------------------------------------------------------------------------
// acc: per pixel {A_r, A_g, A_b, S} uint64.  Every lane of a wave reaches the ballots (no early return).
__global__ void __launch_bounds__(RT) k_splat(Cameras cam, const float* __restrict__ pts, long long ps, long long cs,
                                              const float* __restrict__ colors, int N, int W, int H, float zt,
                                              const uint32_t* __restrict__ zmin, unsigned long long* __restrict__ acc)
{
    const int i = blockIdx.x * RT + threadIdx.x;
    const int f = blockIdx.y;
    const size_t HW = (size_t)W * H;
    const uint32_t* zplane = zmin + (size_t)f * HW;
    unsigned long long* aplane = acc + (size_t)f * HW * 4;
    Projected p;
    p.valid = false;
    p.u = p.v = 0.0;
    p.z = 0.f;
    if (i < N) p = project_point(cam, f, pts, ps, cs, i, W, H);
    const unsigned long long act = __ballot(p.valid);
    if (act == 0ull) return;                                  // wave-uniform

    unsigned long long cq[3] = { 0ull, 0ull, 0ull };
    if (p.valid) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float v = colors[(size_t)i * 3 + c];
            v = v > 0.f ? v : 0.f;                            // NaN -> 0
            v = v < 1.f ? v : 1.f;
            cq[c] = (unsigned long long)rint((double)v * 65535.0);
        }
    }
    const double fx0 = floor(p.u), fy0 = floor(p.v);
    const double fx = p.u - fx0, fy = p.v - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    unsigned long long wq[4];
    int pixn[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int dx = k & 1, dy = k >> 1;
        const double w = (dx ? fx : 1.0 - fx) * (dy ? fy : 1.0 - fy);
        const int xx = x0 + dx, yy = y0 + dy;
        const bool inside = p.valid && xx <= W - 1 && yy <= H - 1;
        pixn[k] = inside ? yy * W + xx : 0;
        unsigned long long q = 0ull;
        if (inside) {
            const uint32_t zb = zplane[pixn[k]];
            const float zm = zb == NO_HIT ? __uint_as_float(0x7f800000u) : __uint_as_float(zb);
            if (p.z <= zm * zt) q = (unsigned long long)rint(w * 65536.0);
        }
        wq[k] = q;
    }
    const int cell = y0 * W + x0;
    const int first = __ffsll((long long)act) - 1;
    const int cell0 = __shfl(cell, first);
    if (__popcll(act) > 1 && __ballot(p.valid && cell == cell0) == act) {
        // the whole wave in one bilinear cell: sum on chip, one lane adds.  The neighbour indices are the first lane's.
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long s = wave_sum(wq[k]);
            const unsigned long long a0 = wave_sum(wq[k] * cq[0]);
            const unsigned long long a1 = wave_sum(wq[k] * cq[1]);
            const unsigned long long a2 = wave_sum(wq[k] * cq[2]);
            if ((int)__lane_id() == first && s != 0ull) {
                unsigned long long* a = aplane + (size_t)pixn[k] * 4;
                atomicAdd(a + 0, a0);
                atomicAdd(a + 1, a1);
                atomicAdd(a + 2, a2);
                atomicAdd(a + 3, s);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (wq[k] == 0ull) continue;
            unsigned long long* a = aplane + (size_t)pixn[k] * 4;
            atomicAdd(a + 0, wq[k] * cq[0]);
            atomicAdd(a + 1, wq[k] * cq[1]);
            atomicAdd(a + 2, wq[k] * cq[2]);
            atomicAdd(a + 3, wq[k]);
        }
    }
}

// ---- dilation / erosion ------------------------------------------------------------------------------------------------------
// One workgroup forms a WT_X x WT_Y tile of the output from the tile and its halo of R pixels: rows first, then columns.
// Pixels outside the image hold the operation's neutral element, which is what a window clamped to the image amounts to.
constexpr int WT_X = 64, WT_Y = 16;

template <int R, bool IS_MAX, bool FROM_ZMIN>
__global__ void __launch_bounds__(RT) k_window(const void* __restrict__ src_, uint8_t* __restrict__ dst, int W, int H)
{
    constexpr int SX = WT_X + 2 * R, SY = WT_Y + 2 * R;
    constexpr uint8_t NEUTRAL = IS_MAX ? 0 : 1;
    __shared__ uint8_t s_in[SY][SX];
    __shared__ uint8_t s_row[SY][WT_X];
    const size_t HW = (size_t)W * H;
    const int f = blockIdx.z;
    const int bx = blockIdx.x * WT_X, by = blockIdx.y * WT_Y;
    for (int t = threadIdx.x; t < SX * SY; t += RT) {
        const int ly = t / SX, lx = t - ly * SX;
        const int gx = bx + lx - R, gy = by + ly - R;
        uint8_t v = NEUTRAL;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)f * HW + (size_t)gy * W + gx;
            v = FROM_ZMIN ? (uint8_t)(static_cast<const uint32_t*>(src_)[g] != NO_HIT) : static_cast<const uint8_t*>(src_)[g];
        }
        s_in[ly][lx] = v;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < SY * WT_X; t += RT) {
        const int ly = t / WT_X, lx = t - ly * WT_X;
        uint8_t v = NEUTRAL;
#pragma unroll
        for (int d = 0; d <= 2 * R; d++) v = IS_MAX ? (uint8_t)(v | s_in[ly][lx + d]) : (uint8_t)(v & s_in[ly][lx + d]);
        s_row[ly][lx] = v;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < WT_Y * WT_X; t += RT) {
        const int ly = t / WT_X, lx = t - ly * WT_X;
        const int gx = bx + lx, gy = by + ly;
        if (gx >= W || gy >= H) continue;
        uint8_t v = NEUTRAL;
#pragma unroll
        for (int d = 0; d <= 2 * R; d++) v = IS_MAX ? (uint8_t)(v | s_row[ly + d][lx]) : (uint8_t)(v & s_row[ly + d][lx]);
        dst[(size_t)f * HW + (size_t)gy * W + gx] = v;
    }
}

// ---- resolve -----------------------------------------------------------------------------------------------------------------
// grid (ceil(HW / RT), frames).  Outputs are optional.
__global__ void __launch_bounds__(RT) k_resolve(int W, int H, const uint32_t* __restrict__ zmin,
                                                const unsigned long long* __restrict__ acc, const uint8_t* __restrict__ dil,
                                                const uint8_t* __restrict__ mask, int with_image, float* __restrict__ out_image,
                                                uint8_t* __restrict__ out_u8, uint8_t* __restrict__ out_mask,
                                                uint8_t* __restrict__ out_dil, uint8_t* __restrict__ out_border,
                                                float* __restrict__ out_depth)
{
    const int HW = W * H;
    const int p = blockIdx.x * RT + threadIdx.x;
    if (p >= HW) return;
    const size_t base = (size_t)blockIdx.y * HW;
    const uint8_t* mplane = mask + base;
    const uint8_t m = mplane[p];
    const int y = p / W, x = p - y * W;
    if (out_mask) out_mask[base + p] = m;
    if (out_dil) out_dil[base + p] = dil[base + p];
    if (out_border) {
        // mask_hf of R/luciddreamer.py:411-413: differences to the pixel below and to the right, last row / column repeated
        const int yc = y < H - 1 ? y : H - 2, xc = x < W - 1 ? x : W - 2;
        const uint8_t c = mplane[yc * W + xc];
        out_border[base + p] = (uint8_t)(c != mplane[(yc + 1) * W + xc] || c != mplane[yc * W + xc + 1]);
    }
    if (out_depth) {
        const uint32_t zb = zmin[base + p];
        out_depth[base + p] = (m && zb < 0x7f800000u) ? __uint_as_float(zb) : 0.f;
    }
    if (!with_image) return;
    float rgb[3] = { 0.f, 0.f, 0.f };
    if (m) {
        const unsigned long long* aplane = acc + base * 4;
        unsigned long long a[4];
#pragma unroll
        for (int c = 0; c < 4; c++) a[c] = aplane[(size_t)p * 4 + c];
        if (a[3] == 0ull) {
            // no accepted contribution: the integer sums over the clamped 9x9 window (non-zero: the pixel is in `dil`)
            const int ys = y - DIL_R > 0 ? y - DIL_R : 0, ye = y + DIL_R < H - 1 ? y + DIL_R : H - 1;
            const int xs = x - DIL_R > 0 ? x - DIL_R : 0, xe = x + DIL_R < W - 1 ? x + DIL_R : W - 1;
            for (int yy = ys; yy <= ye; yy++)
                for (int xx = xs; xx <= xe; xx++) {
                    const unsigned long long* q = aplane + ((size_t)yy * W + xx) * 4;
#pragma unroll
                    for (int c = 0; c < 4; c++) a[c] += q[c];
                }
        }
        const double s = (double)a[3];
#pragma unroll
        for (int c = 0; c < 3; c++) rgb[c] = (float)(((double)a[c] / s) / 65535.0);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (out_image) out_image[(base + p) * 3 + c] = rgb[c];
        if (out_u8) out_u8[(base + p) * 3 + c] = (uint8_t)rintf(rgb[c] * 255.f);
    }
}

// ---- lift --------------------------------------------------------------------------------------------------------------------
struct LiftMats { double Kinv[9], Rinv[9], t[3]; };

__global__ void __launch_bounds__(RT) k_lift(LiftMats m, int W, int H, const float* __restrict__ depth, float* __restrict__ out)
{
    const int HW = W * H;
    const int p = blockIdx.x * RT + threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    const double d = (double)depth[p];
    const double xd = (double)x * d, yd = (double)y * d;
    const double c0 = row3(m.Kinv, xd, yd, d), c1 = row3(m.Kinv + 3, xd, yd, d), c2 = row3(m.Kinv + 6, xd, yd, d);
    out[p] = (float)(row3(m.Rinv, c0, c1, c2) - m.t[0]);
    out[(size_t)HW + p] = (float)(row3(m.Rinv + 3, c0, c1, c2) - m.t[1]);
    out[2 * (size_t)HW + p] = (float)(row3(m.Rinv + 6, c0, c1, c2) - m.t[2]);
}

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Layout { size_t acc, zmin, dil, mask, total; };

inline Layout layout(int n_frames, size_t HW)
{
    Layout l;
    const size_t F = (size_t)n_frames;
    l.acc = 0;
    l.zmin = l.acc + align256(F * HW * 32);
    l.dil = l.zmin + align256(F * HW * 4);
    l.mask = l.dil + align256(F * HW);
    l.total = l.mask + align256(F * HW);
    return l;
}

}  // namespace

size_t reproject_workspace_bytes(int n_frames, int height, int width)
{
    return layout(n_frames, (size_t)height * width).total;
}

hipError_t launch_reproject(const ReprojectLaunch& a, hipStream_t s)
{
    const size_t HW = (size_t)a.height * a.width;
    const Layout l = layout(a.n_frames, HW);
    char* ws = static_cast<char*>(a.workspace);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(ws + l.acc);
    uint32_t* zmin = reinterpret_cast<uint32_t*>(ws + l.zmin);
    uint8_t* dil = reinterpret_cast<uint8_t*>(ws + l.dil);
    uint8_t* mask = reinterpret_cast<uint8_t*>(ws + l.mask);
    const bool with_image = a.out_image || a.out_image_u8;
    const size_t F = (size_t)a.n_frames;
    hipError_t e = hipMemsetAsync(zmin, 0xFF, F * HW * 4, s);
    if (e != hipSuccess) return e;
    if (with_image) {
        e = hipMemsetAsync(acc, 0, F * HW * 32, s);
        if (e != hipSuccess) return e;
    }
    const float zt = 1.0f + a.z_tolerance;
    const unsigned pblocks = (unsigned)(((long long)a.n_points + RT - 1) / RT);
    for (int f0 = 0; f0 < a.n_frames && pblocks > 0; f0 += REPROJECT_FRAMES_PER_LAUNCH) {
        const int nf = a.n_frames - f0 < REPROJECT_FRAMES_PER_LAUNCH ? a.n_frames - f0 : REPROJECT_FRAMES_PER_LAUNCH;
        Cameras cam;
        for (int k = 0; k < 9; k++) cam.K[k] = a.K[k];
        for (int f = 0; f < REPROJECT_FRAMES_PER_LAUNCH; f++) {
            const int g = f < nf ? f0 + f : f0;
            for (int k = 0; k < 9; k++) cam.R[f][k] = a.R[(size_t)g * 9 + k];
            for (int k = 0; k < 3; k++) cam.T[f][k] = a.T[(size_t)g * 3 + k];
        }
        const dim3 grid(pblocks, (unsigned)nf);
        k_project<<<grid, RT, 0, s>>>(cam, a.points, a.point_stride, a.coord_stride, a.n_points, a.width, a.height,
                                      zmin + (size_t)f0 * HW, a.out_valid, a.out_pix);
    }
    if (with_image) {
        // the splat reads final zmin planes: behind every project launch of its frames (stream order)
        for (int f0 = 0; f0 < a.n_frames && pblocks > 0; f0 += REPROJECT_FRAMES_PER_LAUNCH) {
            const int nf = a.n_frames - f0 < REPROJECT_FRAMES_PER_LAUNCH ? a.n_frames - f0 : REPROJECT_FRAMES_PER_LAUNCH;
            Cameras cam;
            for (int k = 0; k < 9; k++) cam.K[k] = a.K[k];
            for (int f = 0; f < REPROJECT_FRAMES_PER_LAUNCH; f++) {
                const int g = f < nf ? f0 + f : f0;
                for (int k = 0; k < 9; k++) cam.R[f][k] = a.R[(size_t)g * 9 + k];
                for (int k = 0; k < 3; k++) cam.T[f][k] = a.T[(size_t)g * 3 + k];
            }
            const dim3 grid(pblocks, (unsigned)nf);
            k_splat<<<grid, RT, 0, s>>>(cam, a.points, a.point_stride, a.coord_stride, a.colors, a.n_points, a.width, a.height,
                                        zt, zmin + (size_t)f0 * HW, acc + (size_t)f0 * HW * 4);
        }
    }
    // blockIdx.z carries the frame of the window kernels: at most 65535 per launch
    const unsigned tx = (unsigned)((a.width + WT_X - 1) / WT_X), ty = (unsigned)((a.height + WT_Y - 1) / WT_Y);
    for (int f0 = 0; f0 < a.n_frames; f0 += 65535) {
        const unsigned nf = (unsigned)(a.n_frames - f0 < 65535 ? a.n_frames - f0 : 65535);
        const dim3 grid(tx, ty, nf);
        k_window<DIL_R, true, true><<<grid, RT, 0, s>>>(zmin + (size_t)f0 * HW, dil + (size_t)f0 * HW, a.width, a.height);
        k_window<ERO_R, false, false><<<grid, RT, 0, s>>>(dil + (size_t)f0 * HW, mask + (size_t)f0 * HW, a.width, a.height);
    }
    const unsigned qblocks = (unsigned)((HW + RT - 1) / RT);
    for (int f0 = 0; f0 < a.n_frames; f0 += 65535) {
        const unsigned nf = (unsigned)(a.n_frames - f0 < 65535 ? a.n_frames - f0 : 65535);
        const size_t o = (size_t)f0 * HW;
        k_resolve<<<dim3(qblocks, nf), RT, 0, s>>>(a.width, a.height, zmin + o, acc + o * 4, dil + o, mask + o, with_image ? 1 : 0,
                                                   a.out_image ? a.out_image + o * 3 : nullptr,
                                                   a.out_image_u8 ? a.out_image_u8 + o * 3 : nullptr,
                                                   a.out_mask ? a.out_mask + o : nullptr, a.out_dilated ? a.out_dilated + o : nullptr,
                                                   a.out_border ? a.out_border + o : nullptr, a.out_depth ? a.out_depth + o : nullptr);
    }
    return hipGetLastError();
}

hipError_t launch_lift(int height, int width, const float* depth, const double* Kinv, const double* Rinv, const double* RinvT,
                       float* out, hipStream_t s)
{
    LiftMats m;
    for (int k = 0; k < 9; k++) { m.Kinv[k] = Kinv[k]; m.Rinv[k] = Rinv[k]; }
    for (int k = 0; k < 3; k++) m.t[k] = RinvT[k];
    const size_t HW = (size_t)height * width;
    k_lift<<<(unsigned)((HW + RT - 1) / RT), RT, 0, s>>>(m, width, height, depth, out);
    return hipGetLastError();
}

}  // namespace lr
