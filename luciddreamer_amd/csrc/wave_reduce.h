// wave_reduce.h -- the wave64 reduction pieces the per-tile backward kernels share (render_bwd.hip, render_distort.hip), for gfx950:
// DPP moves, the sum over a 16-lane row, the whole-wave sum, and the lane-swap reduction of eight terms down to rows.  What a kernel does with the row
// partials (render_bwd.hip: row_merge3 / lds_reduce9; render_distort.hip: two row sums) stays with the kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace lr {

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
// sum within each 16-lane row; every lane of the row ends with the row total
__device__ __forceinline__ float row_sum(float v)
{
    v += dpp<0xB1>(v);
    v += dpp<0x4E>(v);
    v += dpp<0x141>(v);
    v += dpp<0x140>(v);
    return v;
}
// sum over the wave's 64 lanes in a fixed order (xor butterfly 32, 16, ..., 1); every lane ends with the total.  The double
// form is what the loss kernels reduce their per-lane sums with (smooth.hip).
template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// (inline asm below: with ROCm 7.2 hipcc, __builtin_amdgcn_permlane32_swap followed by r[0] + r[1] returned 2 * r[0] --
//  verified on hardware)
// Reduce eight per-lane terms over the wave down to 16-lane rows: on return row r of `a0` holds the row partials of term
// {a0, a2, a1, a3}[r] and row r of `b0` those of {b0, b2, b1, b3}[r]; a row_sum of each finishes the job.  One asm block so
// that the six swaps share two hazard waits instead of paying one each (VALU write -> v_permlane*_swap read needs two
// wait states, swap -> VALU read one; every dependent pair below has that many instructions in between):
//   4 x [x <- (lanes<32: x[l] + x[l+32]) | (lanes>=32: y[l-32] + y[l])]   then   2 x the same over 16-lane rows
__device__ __forceinline__ void reduce8(float& a0, float a1, float a2, float a3, float& b0, float b1, float b2, float b3)
{
    asm volatile("s_nop 1\n\t"
                 "v_permlane32_swap_b32 %0, %1\n\t"
                 "v_permlane32_swap_b32 %2, %3\n\t"
                 "v_permlane32_swap_b32 %4, %5\n\t"
                 "v_permlane32_swap_b32 %6, %7\n\t"
                 "v_add_f32 %0, %0, %1\n\t"
                 "v_add_f32 %2, %2, %3\n\t"
                 "v_add_f32 %4, %4, %5\n\t"
                 "v_add_f32 %6, %6, %7\n\t"
                 "v_permlane16_swap_b32 %0, %2\n\t"
                 "s_nop 0\n\t"
                 "v_permlane16_swap_b32 %4, %6\n\t"
                 "v_add_f32 %0, %0, %2\n\t"
                 "v_add_f32 %4, %4, %6\n\t"
                 "s_nop 1"                                  // whatever follows may be a DPP read of %0 / %4 (two wait states)
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));
}

}  // namespace lr
