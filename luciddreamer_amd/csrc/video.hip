// video.hip -- the per-frame post-processing of the video renderer (R/luciddreamer.py:250-265) for gfx950.
//
// The reference turns every rendered frame into bytes on the host:
//     frame : np.round(image.permute(1,2,0).cpu().numpy().clip(0,1) * 255.).astype(np.uint8)
//     depth : colorize(-(depth * (depth > 0)).cpu().numpy())          (R/utils/depth.py: percentiles 2 / 98 over the valid
//             pixels, normalise, matplotlib colormap lookup with bytes=True, background colour for invalid pixels)
// Here the same bytes are formed on the device, every frame of a batch in the same launches:
//   k_frames_u8      : CHW float32 -> HWC uint8, four pixels (16 B of each channel plane) per lane, 12 B stored packed.
//   k_sel_hist<P>    : pass P of a 3-pass radix select (11 / 11 / 10 bits) over order-preserving uint32 keys of the valid
//                      values: per-workgroup LDS histograms merged into the frame's histogram with integer atomics only
//                      (the result does not depend on arrival order).  Pass 1 also counts NaNs and invalid pixels.  Passes 2
//                      and 3 count only keys under the prefixes still open, one histogram per DISTINCT prefix.
//   k_sel_narrow<P>  : one workgroup per frame.  After pass 1 it forms n and the four ranks (lo / hi of both percentiles, the
//                      numpy "linear" method in float32) on the device; after every pass it narrows each rank's prefix by
//                      the histogram; after pass 3 it forms vmin / vmax exactly as numpy's float32 np.percentile does.
//   k_depth_colorize : the negation, the normalisation, the colormap gather from an LDS copy of the (N+3)-row LUT, the
//                      background of invalid pixels, packed 4-byte RGBA stores.
// Nothing reads back to the host.  The TU is compiled with -ffp-contract=off: every float operation above is one IEEE float32
// operation, as numpy performs it.
#include "common.h"
#include "lucid_raster.h"

namespace lr {

namespace {

constexpr int VT = 256;                     // threads per workgroup of every kernel here
constexpr int B1 = 2048, B2 = 2048, B3 = 1024;   // 11 / 11 / 10 key bits per pass
constexpr int NT = 4;                       // order statistics selected together: lo, hi of q_lo; lo, hi of q_hi
constexpr int MAX_SEL_BLOCKS = 512;         // histogram workgroups per frame

// per-frame select state at the head of the frame's workspace slab (uint32 words)
struct SelState {
    uint32_t n_nan, n_invalid, done, pad0;  // done: 1 = vmin / vmax already final (n == 0, or a NaN among the valid values)
    uint32_t prefix[NT];                    // key bits selected so far (high bits first)
    uint32_t rank[NT];                      // rank of the target among the keys that share its prefix
    uint32_t slot[NT];                      // histogram of the next pass this target reads (first target with its prefix)
    float g[2];                             // interpolation weights of q_lo, q_hi
    uint32_t pad1[14];
};
static_assert(sizeof(SelState) == 32 * 4, "SelState is 32 words");
constexpr size_t FRAME_WORDS = 32 + B1 + NT * B2 + NT * B3;

__device__ __forceinline__ SelState* sel_state(uint32_t* ws, int f) { return reinterpret_cast<SelState*>(ws + (size_t)f * FRAME_WORDS); }
__device__ __forceinline__ uint32_t* sel_hist(uint32_t* ws, int f, int pass)
{
    uint32_t* h = ws + (size_t)f * FRAME_WORDS + 32;
    return pass == 1 ? h : pass == 2 ? h + B1 : h + B1 + NT * B2;
}

__device__ __forceinline__ uint32_t to_u8(float x)
{
    float c = x > 0.f ? x : 0.f;            // NaN -> 0
    c = c < 1.f ? c : 1.f;
    return (uint32_t)rintf(c * 255.f);      // round half to even, as np.round
}

// the value colorize() sees: -(d * (d > 0)) as torch computes it (d <= 0 -> -0.0, -inf -> NaN, NaN stays NaN), or d itself
__device__ __forceinline__ float depth_value(float d, bool from_render)
{
    if (!from_render) return d;
    const float m = d > 0.f ? 1.f : 0.f;
    return -(d * m);
}

// order-preserving key of a non-NaN float; -0.0 and +0.0 share one key
__device__ __forceinline__ uint32_t order_key(float v)
{
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float key_value(uint32_t k)
{
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
#endif
}

// one LDS histogram increment per active lane.  Heavily tied data (a background of -0.0, constant maps) sends a whole wave to
// one bin: then one lane adds the wave's count instead of 64 lanes serialising on one address.  Called by every lane of the wave.
__device__ __forceinline__ void hist_add(uint32_t* h, uint32_t bin, bool active)
{
    const unsigned long long act = __ballot(active);
    if (act == 0ull) return;
    const int first = __ffsll((long long)act) - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)bin, first);
    const unsigned long long same = __ballot(active && bin == b0);
    if (same == act) {
        if ((int)__lane_id() == first) atomicAdd(&h[b0], (uint32_t)__popcll(act));
    } else if (active) {
        atomicAdd(&h[bin], 1u);
    }
}

// four consecutive pixels of one plane (q = quad index); lanes past the plane's end read NaN-free zeros and report !ok
template <bool VEC>
__device__ __forceinline__ void load4(const float* plane, int HW, int q, float v[4], bool ok[4])
{
    const int p = q * 4;
    if (VEC) {
        const float4 t = (p < HW) ? *reinterpret_cast<const float4*>(plane + p) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
#pragma unroll
        for (int j = 0; j < 4; j++) ok[j] = p < HW;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            ok[j] = p + j < HW;
            v[j] = ok[j] ? plane[p + j] : 0.f;
        }
    }
}

// ---- frames ---------------------------------------------------------------------------------------------------------------
// grid (ceil(quads / VT), n_frames); VEC: H*W % 4 == 0 and 16-byte aligned planes (every frame of a contiguous batch then is)
template <bool VEC>
__global__ void __launch_bounds__(VT) k_frames_u8(const float* __restrict__ img, uint8_t* __restrict__ out, int HW)
{
    const int q = blockIdx.x * VT + threadIdx.x;
    const int p = q * 4;
    if (p >= HW) return;
    const float* src = img + (size_t)blockIdx.y * 3 * HW;
    uint8_t* dst = out + (size_t)blockIdx.y * 3 * HW;
    if (VEC) {
        const float4 r = *reinterpret_cast<const float4*>(src + p);
        const float4 g = *reinterpret_cast<const float4*>(src + HW + p);
        const float4 b = *reinterpret_cast<const float4*>(src + 2 * HW + p);
        const uint32_t w0 = to_u8(r.x) | to_u8(g.x) << 8 | to_u8(b.x) << 16 | to_u8(r.y) << 24;
        const uint32_t w1 = to_u8(g.y) | to_u8(b.y) << 8 | to_u8(r.z) << 16 | to_u8(g.z) << 24;
        const uint32_t w2 = to_u8(b.z) | to_u8(r.w) << 8 | to_u8(g.w) << 16 | to_u8(b.w) << 24;
        uint32_t* o = reinterpret_cast<uint32_t*>(dst + 3 * (size_t)p);
        o[0] = w0; o[1] = w1; o[2] = w2;
    } else {
        for (int j = 0; j < 4 && p + j < HW; j++) {
#pragma unroll
            for (int c = 0; c < 3; c++) dst[3 * (size_t)(p + j) + c] = (uint8_t)to_u8(src[(size_t)c * HW + p + j]);
        }
    }
}

// ---- select: histogram passes ----------------------------------------------------------------------------------------------
// grid (blocks per frame, n_frames).  The loop runs the same trip count on every lane (hist_add is a wave operation).
template <int PASS, bool VEC>
__global__ void __launch_bounds__(VT) k_sel_hist(const float* __restrict__ depths, int HW, int from_render, float invalid_val,
                                                 uint32_t* __restrict__ ws)
{
    constexpr int BINS = PASS == 1 ? B1 : PASS == 2 ? B2 : B3;
    constexpr int NH = PASS == 1 ? 1 : NT;
    __shared__ uint32_t s_hist[NH * BINS];
    __shared__ uint32_t s_cnt[2];
    const int f = blockIdx.y;
    SelState* st = sel_state(ws, f);
    uint32_t pre[NT];
    bool own[NT];
    if (PASS > 1) {
        if (st->done) return;                               // uniform: the frame's vmin / vmax are already final
#pragma unroll
        for (int t = 0; t < NT; t++) { pre[t] = st->prefix[t]; own[t] = st->slot[t] == (uint32_t)t; }
    }
    for (int i = threadIdx.x; i < NH * BINS; i += VT) s_hist[i] = 0u;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
    __syncthreads();

    const float* plane = depths + (size_t)f * HW;
    const int nq = (HW + 3) / 4;
    uint32_t n_nan = 0, n_inv = 0;
    for (int base = blockIdx.x * VT; base < nq; base += gridDim.x * VT) {
        float v[4];
        bool ok[4];
        load4<VEC>(plane, HW, base + threadIdx.x, v, ok);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float x = depth_value(v[j], from_render != 0);
            const bool inv = ok[j] && x == invalid_val;
            const bool nan = ok[j] && x != x;
            const bool val = ok[j] && !inv && !nan;
            const uint32_t k = val ? order_key(x) : 0u;
            if (PASS == 1) {
                n_nan += nan;
                n_inv += inv;
                hist_add(s_hist, k >> 21, val);
            } else {
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    if (!own[t]) continue;                  // uniform
                    const bool m = PASS == 2 ? (k >> 21) == pre[t] : (k >> 10) == pre[t];
                    hist_add(s_hist + t * BINS, PASS == 2 ? (k >> 10) & 0x7ffu : k & 0x3ffu, val && m);
                }
            }
        }
    }
    if (PASS == 1) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { n_nan += __shfl_xor(n_nan, off); n_inv += __shfl_xor(n_inv, off); }
        if ((threadIdx.x & 63) == 0) {
            if (n_nan) atomicAdd(&s_cnt[0], n_nan);
            if (n_inv) atomicAdd(&s_cnt[1], n_inv);
        }
    }
    __syncthreads();
    uint32_t* g = sel_hist(ws, f, PASS);
    for (int i = threadIdx.x; i < NH * BINS; i += VT) {
        const uint32_t c = s_hist[i];
        if (c) atomicAdd(&g[i], c);
    }
    if (PASS == 1 && threadIdx.x == 0) {
        if (s_cnt[0]) atomicAdd(&st->n_nan, s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&st->n_invalid, s_cnt[1]);
    }
}

// exclusive prefix sum of one value per thread over the workgroup; *total = the sum of all
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* s_wave, uint32_t* total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    __syncthreads();
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < VT / 64; i++) {
        const uint32_t s = s_wave[i];
        before += i < w ? s : 0u;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

// numpy's float32 "linear" percentile: the virtual index and its interpolation weight
__device__ __forceinline__ void virtual_index(uint32_t n, float q, uint32_t* lo, uint32_t* hi, float* g)
{
    const float q32 = q / 100.f;
    const float vi = (float)(n - 1) * q32;
    float fl = floorf(vi);
    uint32_t l = (uint32_t)fl;
    if (l > n - 1) { l = n - 1; fl = (float)l; }
    *lo = l;
    *hi = l + 1 < n ? l + 1 : n - 1;
    *g = vi - fl;
}

__device__ __forceinline__ float lerp_np(float a, float b, float g)
{
    const float d = b - a;
    return g >= 0.5f ? b - d * (1.f - g) : a + d * g;
}

// ---- select: narrowing, one workgroup per frame -----------------------------------------------------------------------------
template <int PASS>
__global__ void __launch_bounds__(VT) k_sel_narrow(uint32_t* __restrict__ ws, float q_lo, float q_hi,
                                                   float* __restrict__ out_vmm)
{
    constexpr int BINS = PASS == 1 ? B1 : PASS == 2 ? B2 : B3;
    constexpr int PER = BINS / VT;
    constexpr int SHIFT = PASS == 3 ? 10 : 11;
    __shared__ uint32_t s_wave[VT / 64];
    __shared__ uint32_t s_rank[NT], s_pre[NT];
    __shared__ uint32_t s_n;
    const int f = blockIdx.x;
    SelState* st = sel_state(ws, f);
    if (st->done) return;                                   // uniform
    const uint32_t* hist = sel_hist(ws, f, PASS);
    if (PASS == 1) {
        // n = keys histogrammed + NaNs; the ranks of the four order statistics
        uint32_t c = 0;
        for (int j = 0; j < PER; j++) c += hist[threadIdx.x * PER + j];
        uint32_t total;
        block_exclusive_scan(c, s_wave, &total);
        if (threadIdx.x == 0) {
            const uint32_t n = total + st->n_nan;
            s_n = n;
            if (n == 0u || st->n_nan) {
                // no valid pixel (our documented difference: the reference raises IndexError), or numpy's NaN result
                const float nanv = __uint_as_float(0x7fc00000u);
                out_vmm[2 * f] = nanv;
                out_vmm[2 * f + 1] = nanv;
                st->done = 1u;
            } else {
                uint32_t lo, hi;
                float g;
                virtual_index(n, q_lo, &lo, &hi, &g);
                s_rank[0] = lo; s_rank[1] = hi; st->g[0] = g;
                virtual_index(n, q_hi, &lo, &hi, &g);
                s_rank[2] = lo; s_rank[3] = hi; st->g[1] = g;
            }
        }
        __syncthreads();
        if (s_n == 0u || st->n_nan) return;                 // uniform
    } else {
        if (threadIdx.x < NT) { s_rank[threadIdx.x] = st->rank[threadIdx.x]; s_pre[threadIdx.x] = st->prefix[threadIdx.x]; }
        __syncthreads();
    }
    uint32_t slot[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) slot[t] = PASS == 1 ? 0u : st->slot[t];
    __syncthreads();
    for (int t = 0; t < NT; t++) {
        const uint32_t* h = hist + slot[t] * BINS;
        uint32_t c[PER], sum = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) { c[j] = h[threadIdx.x * PER + j]; sum += c[j]; }
        uint32_t total;
        uint32_t cum = block_exclusive_scan(sum, s_wave, &total);
        const uint32_t r = s_rank[t];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; j++) {
            if (r >= cum && r < cum + c[j]) {               // exactly one thread: the bin that holds rank r
                const uint32_t bin = threadIdx.x * PER + j;
                s_rank[t] = r - cum;
                s_pre[t] = PASS == 1 ? bin : (s_pre[t] << SHIFT) | bin;
            }
            cum += c[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (PASS < 3) {
            for (int t = 0; t < NT; t++) {
                st->prefix[t] = s_pre[t];
                st->rank[t] = s_rank[t];
                uint32_t sl = t;
                for (int u = t - 1; u >= 0; u--)
                    if (s_pre[u] == s_pre[t]) sl = u;
                st->slot[t] = sl;
            }
        } else {
            const float a0 = key_value(s_pre[0]), b0 = key_value(s_pre[1]);
            const float a1 = key_value(s_pre[2]), b1 = key_value(s_pre[3]);
            out_vmm[2 * f] = lerp_np(a0, b0, st->g[0]);
            out_vmm[2 * f + 1] = lerp_np(a1, b1, st->g[1]);
        }
    }
}

// ---- colorize ---------------------------------------------------------------------------------------------------------------
constexpr int MAX_LUT_ROWS = LR_VIDEO_MAX_LUT_N + 3;

template <bool VEC>
__global__ void __launch_bounds__(VT) k_depth_colorize(const float* __restrict__ depths, int HW, int from_render,
                                                       float invalid_val, const float* __restrict__ vmm,
                                                       const uint32_t* __restrict__ lut, int lut_n, uint32_t background,
                                                       uint32_t* __restrict__ out)
{
    __shared__ uint32_t s_lut[MAX_LUT_ROWS];
    for (int i = threadIdx.x; i < lut_n + 3; i += VT) s_lut[i] = lut[i];
    __syncthreads();
    const int f = blockIdx.y;
    const int q = blockIdx.x * VT + threadIdx.x;
    if (q * 4 >= HW) return;
    const float vmin = vmm[2 * f], vmax = vmm[2 * f + 1];
    const bool scale = vmin != vmax;                        // NaN != NaN: the NaN limits reach every pixel, as in numpy
    const float range = vmax - vmin;
    const float fn = (float)lut_n;
    float v[4];
    bool ok[4];
    load4<VEC>(depths + (size_t)f * HW, HW, q, v, ok);
    uint32_t rgba[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float x = depth_value(v[j], from_render != 0);
        const float t = scale ? (x - vmin) / range : x * 0.f;
        float xa = t * fn;
        if (xa == fn) xa = fn - 1.f;
        int idx;
        if (xa != xa) idx = lut_n + 2;                      // bad
        else if (xa < 0.f) idx = lut_n;                     // under
        else if (xa >= fn) idx = lut_n + 1;                 // over
        else idx = (int)xa;
        rgba[j] = x == invalid_val ? background : s_lut[idx];
    }
    uint32_t* o = out + (size_t)f * HW + (size_t)q * 4;
    if (VEC) {
        *reinterpret_cast<uint4*>(o) = make_uint4(rgba[0], rgba[1], rgba[2], rgba[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (ok[j]) o[j] = rgba[j];
    }
}

inline bool vec_ok(int HW, const void* a, const void* b)
{
    return HW % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 15u) == 0 && (reinterpret_cast<uintptr_t>(b) & 15u) == 0;
}

}  // namespace

size_t video_workspace_bytes(int n_frames) { return (size_t)n_frames * FRAME_WORDS * sizeof(uint32_t); }

void launch_frames_u8(int n, int HW, const float* images, uint8_t* out, hipStream_t s)
{
    const dim3 grid((unsigned)((HW + 4 * VT - 1) / (4 * VT)), (unsigned)n);
    // the packed path stores 12 B per lane at 12-byte strides: 4-byte alignment of `out` suffices
    if (HW % 4 == 0 && (reinterpret_cast<uintptr_t>(images) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0)
        k_frames_u8<true><<<grid, VT, 0, s>>>(images, out, HW);
    else
        k_frames_u8<false><<<grid, VT, 0, s>>>(images, out, HW);
}

hipError_t launch_depth_colorize(int n, int HW, const float* depths, bool from_render, float invalid_val, float q_lo,
                                 float q_hi, const float* fixed_vmm, const uint32_t* lut, int lut_n, uint32_t background,
                                 uint32_t* out, float* out_vmm, void* workspace, hipStream_t s)
{
    const bool vec = vec_ok(HW, depths, out);
    const int fr = from_render ? 1 : 0;
    const float* vmm = fixed_vmm;
    if (!fixed_vmm) {
        uint32_t* ws = static_cast<uint32_t*>(workspace);
        hipError_t e = hipMemsetAsync(ws, 0, video_workspace_bytes(n), s);
        if (e != hipSuccess) return e;
        const int nq = (HW + 3) / 4;
        int bpf = (nq + 2 * VT - 1) / (2 * VT);                   // at least two quads (8 pixels) per lane
        bpf = bpf < 1 ? 1 : bpf > MAX_SEL_BLOCKS ? MAX_SEL_BLOCKS : bpf;
        const dim3 hg((unsigned)bpf, (unsigned)n);
        if (vec) k_sel_hist<1, true><<<hg, VT, 0, s>>>(depths, HW, fr, invalid_val, ws);
        else k_sel_hist<1, false><<<hg, VT, 0, s>>>(depths, HW, fr, invalid_val, ws);
        k_sel_narrow<1><<<n, VT, 0, s>>>(ws, q_lo, q_hi, out_vmm);
        if (vec) k_sel_hist<2, true><<<hg, VT, 0, s>>>(depths, HW, fr, invalid_val, ws);
        else k_sel_hist<2, false><<<hg, VT, 0, s>>>(depths, HW, fr, invalid_val, ws);
        k_sel_narrow<2><<<n, VT, 0, s>>>(ws, q_lo, q_hi, out_vmm);
        if (vec) k_sel_hist<3, true><<<hg, VT, 0, s>>>(depths, HW, fr, invalid_val, ws);
        else k_sel_hist<3, false><<<hg, VT, 0, s>>>(depths, HW, fr, invalid_val, ws);
        k_sel_narrow<3><<<n, VT, 0, s>>>(ws, q_lo, q_hi, out_vmm);
        vmm = out_vmm;
    } else if (out_vmm) {
        hipError_t e = hipMemcpyAsync(out_vmm, fixed_vmm, 2 * sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((HW + 4 * VT - 1) / (4 * VT)), (unsigned)n);
    if (vec) k_depth_colorize<true><<<grid, VT, 0, s>>>(depths, HW, fr, invalid_val, vmm, lut, lut_n, background, out);
    else k_depth_colorize<false><<<grid, VT, 0, s>>>(depths, HW, fr, invalid_val, vmm, lut, lut_n, background, out);
    return hipGetLastError();
}

}  // namespace lr
