// mask_scan.h -- the two-kernel exclusive scan over a byte array, shared by rows.hip (row selection: the bytes are a mask) and
// tsdf.hip (mesh extraction: the used-edge mask, and the per-cell triangle counts, whose bytes are the values themselves).
//   k_mask_count   : one sum per workgroup of RS_TILE bytes -> block_counts[blockIdx.x]
//   k_block_prefix : (optional, one workgroup) block_counts[0..n) -> their exclusive prefixes in place, the total -> block_counts[n]
//   k_mask_rank    : rank[i] = sum of the values before i, total -> *out_count
// PRESCANNED = false: every workgroup of k_mask_rank sums the block counts in front of it itself, n^2 / 2 reads over the launch:
// right for rows.hip, whose n is a few thousand at most.  PRESCANNED = true: k_block_prefix ran in between and a workgroup reads
// one word; tsdf.hip scans 7 bytes per lattice point (57 344 workgroups at 256^3, a million at the largest volume).
// COUNTS = false: a byte counts 1 when it is not 0.  COUNTS = true: a byte counts its value.  Sums are uint32.
// The kernels sit in an unnamed namespace: every translation unit that includes this header gets its own copies.
#pragma once
#include "common.h"

namespace lr {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_ITEMS = 8;
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;          // bytes per workgroup

__device__ __forceinline__ uint32_t rs_block_sum(uint32_t v, uint32_t* s_tmp)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    lds_barrier();
    if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
    lds_barrier();
    return s_tmp[0] + s_tmp[1] + s_tmp[2] + s_tmp[3];
}

template <bool COUNTS>
__device__ __forceinline__ uint32_t rs_value(uint8_t b)
{
    return COUNTS ? (uint32_t)b : (b != 0 ? 1u : 0u);
}

template <bool COUNTS>
__global__ void __launch_bounds__(RS_THREADS)
k_mask_count(int P, const uint8_t* __restrict__ mask, uint32_t* __restrict__ block_counts)
{
    __shared__ uint32_t s_tmp[4];
    const int base = blockIdx.x * RS_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < RS_ITEMS; i++) {
        const int k = base + i * RS_THREADS + threadIdx.x;
        if (k < P) c += rs_value<COUNTS>(mask[k]);
    }
    c = rs_block_sum(c, s_tmp);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = c;
}

// block_counts [n + 1]: the n sums become their exclusive prefixes, the total goes to block_counts[n].  ONE workgroup, which
// walks the sums RS_THREADS at a time with a running carry.
__global__ void __launch_bounds__(RS_THREADS) k_block_prefix(int n, uint32_t* __restrict__ block_counts)
{
    __shared__ uint32_t s_wave[4];
    uint32_t carry = 0;
    for (int base = 0; base < n; base += RS_THREADS) {               // uniform over the workgroup
        const int i = base + threadIdx.x;
        const uint32_t v = i < n ? block_counts[i] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(inc, off);
            if ((int)(threadIdx.x & 63) >= off) inc += t;
        }
        const int w = threadIdx.x >> 6;
        lds_barrier();                                               // the previous round's reads of s_wave are done
        if ((threadIdx.x & 63) == 63) s_wave[w] = inc;
        lds_barrier();
        uint32_t wbase = 0;
        for (int k = 0; k < w; k++) wbase += s_wave[k];
        if (i < n) block_counts[i] = carry + wbase + inc - v;
        carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    }
    if (threadIdx.x == 0) block_counts[n] = carry;
}

// rank[i] = sum of the values before i (for a mask: the number of selected rows before i, valid where mask[i] != 0);
// total -> *out_count
template <bool COUNTS, bool PRESCANNED = false>
__global__ void __launch_bounds__(RS_THREADS)
k_mask_rank(int P, const uint8_t* __restrict__ mask, const uint32_t* __restrict__ block_counts,
            uint32_t* __restrict__ rank, int* __restrict__ out_count)
{
    __shared__ uint32_t s_tmp[4];
    __shared__ uint32_t s_wave[4];
    uint32_t pre = 0;
    if (PRESCANNED) {
        pre = block_counts[blockIdx.x];
        if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = (int)block_counts[gridDim.x];
    } else {
        uint32_t all = 0;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += RS_THREADS) {
            const uint32_t v = block_counts[i];
            if (i < (int)blockIdx.x) pre += v;
            all += v;
        }
        pre = rs_block_sum(pre, s_tmp);
        if (blockIdx.x == 0) {
            all = rs_block_sum(all, s_tmp);
            if (threadIdx.x == 0) *out_count = (int)all;
        }
    }
    // blocked arrangement: thread t owns RS_ITEMS consecutive rows
    const int base = blockIdx.x * RS_TILE + threadIdx.x * RS_ITEMS;
    uint32_t flag[RS_ITEMS], sum = 0;
#pragma unroll
    for (int i = 0; i < RS_ITEMS; i++) { flag[i] = base + i < P ? rs_value<COUNTS>(mask[base + i]) : 0u; sum += flag[i]; }
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off);
        if ((int)(threadIdx.x & 63) >= off) inc += t;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) s_wave[w] = inc;
    lds_barrier();
    uint32_t wbase = 0;
    for (int i = 0; i < w; i++) wbase += s_wave[i];
    uint32_t run = pre + wbase + inc - sum;
#pragma unroll
    for (int i = 0; i < RS_ITEMS; i++)
        if (base + i < P) { rank[base + i] = run; run += flag[i]; }
}

}  // namespace

}  // namespace lr
