// render_fwd.hip -- per-tile front-to-back alpha blending with depth output, for gfx950.
//
// Replaces FORWARD::render / renderCUDA (RAST/cuda_rasterizer/forward.cu:261-391).  Per-pixel
// semantics are the reference's exactly (same skip tests, same 0.99 clamp, same T < 1e-4 stop,
// same depth normalisation).  Two kernels with the same results to the bit (launch_render_fwd picks): k_render_fwd below --
// four waves per tile, what a lone view and every small image gets -- and k_render_fwd_tile further down -- one wave per tile, a
// lane owns four pixels, for large images while other views' kernels share the GPU.  k_render_fwd is VALU-issue bound
// (measured: 88 % VALU busy at C3, HBM idle), so its shape is chosen to minimise wave-instructions per pixel x Gaussian pair:
//   * one 256-thread workgroup per 16x16 tile = 4 wave64; a wave owns ONE 8x8 quadrant, a lane one pixel.  (An earlier
//     shape -- 2 waves per tile, two pixels per lane, a candidate stepping only the pixels whose quadrant it hit -- shared
//     the candidate walk and the LDS reads between two quadrants; the quadrant-per-wave shape measured 6 % (C3) to 11 %
//     (dense clouds) faster: a wave walks only its own quadrant's candidates, stops as soon as its own 64 pixels are done,
//     and twice as many waves hide each other's latencies.  A packed FP32 instruction costs twice the issue cycles of a
//     scalar one on MI355X (tools/valu_microbench.hip: 453 vs 912 G wave-instr/s), so packing two pixels buys nothing.)
//     The blend is branch-free: a pixel that skips a Gaussian blends it with weight 0, which is arithmetically identical
//     to the reference's `continue`.
//   * every field the inner loop touches is staged in LDS (the reference re-reads colour and depth
//     from global memory per pixel per Gaussian, forward.cu:359, 364);
//   * two-level loop per wave.  CULL: 64 staged Gaussians at a time, one per LANE, are tested against the
//     wave's 8x8 pixel box with the exact box-minimum of the conic quadratic (common.h box_hit);
//     __ballot turns the result into a 64-bit candidate mask.  BLEND: the wave walks only the set bits
//     (s_ff1), in list order, all lanes evaluating the same Gaussian from broadcast ds_reads.  A
//     non-candidate cannot reach alpha >= 1/255 on any pixel of the box (margin in common.h), so skipping
//     it is exactly the reference's `continue` (forward.cu:338-339).  The outcome per list position and quadrant is left in
//     the binning buffer for the backward, which used to repeat the test;
//   * per-wave early termination via 64-bit __ballot (the reference only stops per block);
//   * tiles are assigned to workgroups so that each XCD (its own 4 MiB L2) renders a contiguous
//     band of the image and re-uses the GaussRecs of Gaussians that straddle neighbouring tiles.
#include "common.h"
#include "dispatch_flags.h"

namespace lr {

namespace {

constexpr int THREADS = 256;        // 4 wave64 per tile
constexpr int NWAVES = THREADS / 64;
constexpr int BATCH = 256;          // staged Gaussians per round = threads per workgroup (14 KB of LDS)

// PixState, pix_start, fwd_pixel, LR_FWD_PARAMS / LR_FWD_PASS and render_fwd_tile (the TILE shape's body): shared with
// render_bwd.hip's fused step kernel
#include "render_fwd_tile_body.h"


// The same step with the candidate's alpha already formed, and branch-free: for the PAIR loop below, where two candidates'
// alphas are evaluated side by side and only these few dependent instructions per candidate remain in sequence.  `enable`:
// all ones, or zero for the second half of an odd pair (the step is then the identity).
template <bool DEPTH, bool COLOR>
__device__ __forceinline__ void fwd_step(PixState<DEPTH, COLOR>& p, uint64_t& done, const float alpha, const float power, const uint64_t enable,
                                         const float cr, const float cg, const float cb, const float depth, const uint32_t pos0)
{
    const float test_T = p.T * (1.0f - alpha);
    const uint64_t pass = enable & ~done & __builtin_amdgcn_ballot_w64(power <= 0.0f) & __builtin_amdgcn_ballot_w64(alpha >= 1.0f / 255.0f);
    const uint64_t low_T = __builtin_amdgcn_ballot_w64(test_T < 0.0001f);
    const uint64_t stop = pass & low_T;
    const bool use = __builtin_amdgcn_inverse_ballot_w64(pass & ~low_T);
    done |= stop;
    if constexpr (COLOR) {
        const float wgt = use ? alpha * p.T : 0.f;
        p.Cr += cr * wgt; p.Cg += cg * wgt; p.Cb += cb * wgt;
        if constexpr (DEPTH) { p.D += depth * wgt; p.acc += wgt; }
    }
    p.T = use ? test_T : p.T;
    p.last = __builtin_amdgcn_inverse_ballot_w64(stop) ? pos0 : p.last;
}

// PAIR: the candidate loop takes two candidates per round (small images: few waves per SIMD, the kernel time is the longest
// wave's dependent chain -- LDS read, exponent, v_exp, the T recursion -- and two candidates' chains overlap except for the
// recursion itself; profiles/r05a_pmc_c5shape.json: VALU busy 49 %, 2.2 waves resident per SIMD on average at 512^2).
// Same operations per pixel and candidate in the same order: bit-identical images.  Per tile: only lists of PAIR_MIN_LIST and more
// (measured, forward alone: dense 512^2, 1 700 per tile, 180 -> 173 us; one layer of pixel-sized splats, 320 per tile, 53.7 -> 55.1).
constexpr int PAIR_MIN_LIST = 1024;
// COLOR = false: out_color is never touched, and the pixel state has no colour channels -- except in the tiles whose list is cut
// into segments: their checkpoints and c_final hold the colour so far, which the backward's segment start reads (render_bwd.hip
// load_pixel).  So such a kernel holds the body twice (render_fwd_quad_body.h: CARRY), and a scalar branch per tile -- the
// length of its list is uniform and known before the first round -- picks the copy.  (The PAIR variant of the diagnostics build
// always carries.)
template <bool STRICT, bool PAIR, bool DEPTH, bool COLOR>
__global__ void __launch_bounds__(THREADS)
k_render_fwd(LR_FWD_PARAMS)
{
    __shared__ float4 s_q0[BATCH];      // x, y, Ap = -0.5 conic a, Bp = -conic b      (common.h gauss_power; x log2 e)
    __shared__ float4 s_q1[BATCH];      // Cp = -0.5 conic c (x log2 e), opacity, depth, qmax (cull threshold, x log2 e)
    __shared__ float4 s_q2[BATCH];      // r, g, b, -
    __shared__ float2 s_q3[BATCH];      // -b/c, -b/a (edge minimiser slopes for box_hit)
    __shared__ int s_wdone[NWAVES];
    __shared__ uint32_t s_seg0;
    if constexpr (COLOR || PAIR) {
        constexpr bool CARRY = true;
#include "render_fwd_quad_body.h"
    } else {
        const int peek = blend_tile(tile_map, num_tiles);
        if (peek < 0) return;
        const uint2 peek_range = ranges[peek];
        if ((int)(peek_range.y - peek_range.x) > BWD_SEG) {
            constexpr bool CARRY = true;
#include "render_fwd_quad_body.h"
        } else {
            constexpr bool CARRY = false;
#include "render_fwd_quad_body.h"
        }
    }
}


// (Round 6 built the producer / consumer split DESIGN.md 8.2 had proposed for small images -- eight waves per tile, per quadrant
//  one wave evaluating alpha into an LDS ring and one carrying the recursion, counters polled with s_sleep -- and removed it again:
//  bit-identical to the quadrant kernel on every test, and 2.2-2.4 x SLOWER (dense 512^2 168 -> 402 us, pixel-sized splats 53 -> 119
//  us): the hand-over costs more instructions than it moves -- VALU 48.6 M -> 131 M, SALU 24.9 M -> 116 M wave-instructions per view,
//  waves parked 140 M -> 554 M cycles (profiles/r06s_ab_fwd_split_dead_end.json, r06t_pmc_c5shape_fwd_*.json; code at commit
//  "Forward split for small images").)

// 64 registers -> 8 waves per SIMD: the 8160 tiles of a 1080p view are all resident at once, as in the backward's TILE shape
// (round 6; with the compiler's own budget, 66-72 registers and 7 waves per SIMD, the last 992 waves waited for the first 7168:
// lone view C3 62.3 -> 59.0 us, C2 101 -> 92 us, dense 1080p 366 -> 342 us, three views in flight equal;
// profiles/r06h_ab_fwdtile8.json).  The quadrant boxes formed per round are what made room (render_fwd_tile).
// (COLOR = false: the two copies of the body and the branch between them, as in k_render_fwd.)
template <bool STRICT, bool DEPTH, bool COLOR>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8), amdgpu_num_vgpr(64)))
k_render_fwd_tile(LR_FWD_PARAMS)
{
    __shared__ float4 s_q0[TSTAGE];     // as in k_render_fwd
    __shared__ float4 s_q1[TSTAGE];
    __shared__ float4 s_q2[TSTAGE];
    if constexpr (COLOR) render_fwd_tile<STRICT, DEPTH, true, true>(LR_FWD_PASS, s_q0, s_q1, s_q2);
    else {
        const int tile = blend_tile(tile_map, num_tiles);
        if (tile < 0) return;
        const uint2 range = ranges[tile];
        if ((int)(range.y - range.x) > BWD_SEG) render_fwd_tile<STRICT, DEPTH, false, true>(LR_FWD_PASS, s_q0, s_q1, s_q2);
        else render_fwd_tile<STRICT, DEPTH, false, false>(LR_FWD_PASS, s_q0, s_q1, s_q2);
    }
}
#undef LR_FWD_PARAMS
#undef LR_FWD_PASS

}  // namespace

void launch_render_fwd(const ViewParams& vp, const GeomView& g, const ImgView& im, const BinView& b, const float* bg,
                       float* out_color, float* out_depth, long long inst_hint, hipStream_t s)
{
    const int gx = vp.gx, gy = vp.gy;
    const int num_tiles = gx * gy;
    if (num_tiles <= 0) return;
    const int tile_map = blend_tile_map(num_tiles);
    const int grid = ((num_tiles + 7) / 8) * 8;
    // Shape (same images, depth, checkpoints and gradients to the bit from all of them):
    //   quadrant kernel (4 waves per tile) -- small images, a lone large view, and large images of long lists;
    //   tile kernel (1 wave per tile) -- large images while other views' kernels are in flight: 10 % fewer VALU instructions and
    //   59 % fewer LDS reads per C3 view (28.7 M -> 25.7 M, 3.10 M -> 1.26 M; profiles/r05x_pmc_fwdtile_*.json).  Three views in
    //   flight, quadrant -> tile kernel (profiles/r06q_shape_sweep.json): C2 +2.5 %, C3 +1 %, 3 M / 1440p (700 instances per
    //   tile) +0.5 %, dense 1 M cloud at 1080p (460 per tile) -1.8 %; a lone view: -2 ... -8 %.  So: large images with other views
    //   in flight, and not on scenes whose earlier views told the host that the lists are longer than a staging round of the
    //   quadrant kernel on average (inst_hint: api.hip view_hint_instances; -1 = unknown).
    //   [Round 5's candidate-PAIR variant of the quadrant kernel (small images, lists of 1024 and more) no longer pays on any
    //    workload of the sweep (-0.5 ... -1.6 %): diagnostics build only.]
    // lr_tune_set("fwd_pair", 0 / 2) forces quadrant / tile (tests, A/B runs); 1 = the pair variant (diagnostics build).
    const int knob = tune_get(TUNE_FWD_PAIR);
    const bool long_lists = inst_hint > (long long)BATCH * num_tiles;
    const bool tile_shape = knob >= 0 ? knob == 2 : (num_tiles > 3072 && views_in_flight() >= 2 && !long_lists);
#ifdef LR_DIAGNOSTICS
    const bool pair = knob == 1;
#else
    constexpr bool pair = false;
#endif
    const bool strict = tune_get(TUNE_STRICT) > 0;
    // out_color == nullptr: the colour-free instantiations, which never touch the pointer.  Only without out_depth: a view that
    // reads its depth keeps carrying the colour and needs an image to write it to (forward_core refuses the combination)
    const bool depth = out_depth != nullptr, color = out_color != nullptr;
    note_fwd_shape(tile_shape ? 2 : pair ? 1 : 0);
    note_fwd_channels((color ? FWD_CHANNEL_COLOR : 0) | (depth ? FWD_CHANNEL_DEPTH : 0));
#define LR_FWD_ARGS 0, s, vp.W, vp.H, gx, num_tiles, tile_map, im.ranges, b.point_list, b.list_gid, g.rec, bg, im.final_T, im.n_contrib, \
                    out_color, out_depth, b.quad_hits, g.header, b.seg_list, b.ckpt, im.tile_seg0, im.c_final
    // out_depth == nullptr: the depth-free instantiations (DEPTH = false never touches the pointer)
    dispatch_flags<3>(flag_bits(strict, depth, color), [&](auto st, auto dp, auto cl) {
        constexpr bool CL = cl.value || dp.value;                         // three channel sets: depth goes with the colour
        if (tile_shape) hipLaunchKernelGGL((k_render_fwd_tile<st.value, dp.value, CL>), dim3(grid), dim3(64), LR_FWD_ARGS);
#ifdef LR_DIAGNOSTICS
        else if (pair) hipLaunchKernelGGL((k_render_fwd<st.value, true, dp.value, CL>), dim3(grid), dim3(THREADS), LR_FWD_ARGS);
#endif
        else hipLaunchKernelGGL((k_render_fwd<st.value, false, dp.value, CL>), dim3(grid), dim3(THREADS), LR_FWD_ARGS);
    });
#undef LR_FWD_ARGS
}

// The alpha output (lr_render_alpha): 1 - T_final of every pixel, from the final_T the blend forward left in the image state --
// a pass of its own, so that the blend-forward kernels stay as they are.  Four pixels per lane when both arrays are 16-byte
// aligned (final_T always is, ImgLayout), else one.
__global__ void __launch_bounds__(256) k_render_alpha(const float* __restrict__ final_T, long long n, float* __restrict__ alpha)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) alpha[i] = 1.0f - final_T[i];
}
__global__ void __launch_bounds__(256) k_render_alpha4(const float4* __restrict__ final_T, long long n4, float4* __restrict__ alpha)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) {
        const float4 t = final_T[i];
        alpha[i] = make_float4(1.0f - t.x, 1.0f - t.y, 1.0f - t.z, 1.0f - t.w);
    }
}

void launch_render_alpha(const float* final_T, long long n, float* alpha, hipStream_t s)
{
    if (n <= 0) return;
    long long done = 0;
    if ((reinterpret_cast<uintptr_t>(alpha) & 15u) == 0 && (reinterpret_cast<uintptr_t>(final_T) & 15u) == 0) {
        const long long n4 = n / 4;
        if (n4 > 0)
            hipLaunchKernelGGL(k_render_alpha4, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                               reinterpret_cast<const float4*>(final_T), n4, reinterpret_cast<float4*>(alpha));
        done = 4 * n4;
    }
    if (done < n)
        hipLaunchKernelGGL(k_render_alpha, dim3((unsigned)((n - done + 255) / 256)), dim3(256), 0, s, final_T + done, n - done,
                           alpha + done);
}

}  // namespace lr
