// tile_sort_small_body.h -- the body of k_tile_sort_small (tilebin.hip), included by the kernels that run it: every bin of up to
// TSORT_GROUP_LDS entries is put in order.  Part A (workgroups below groups4): one wave per bin, which leaves the kernel when its
// bin is done; part B (the others): a whole workgroup per bin of 257..1024 entries, striding over the bins -- these workgroups
// reach the end of the body with all their waves.
// Names the including kernel provides: bins, groups4, sub_shift, slot_bits, num_tiles, bucket_b, rank_max, bin_start, bin_total,
// words, point_list, ranges, inst_gid, list_gid.
    __shared__ __attribute__((aligned(16))) unsigned long long s_a[4 * TSORT_LDS];   // 4 x 256 entries = TSORT_GROUP_LDS
    __shared__ uint32_t s_cnt[TSORT_GROUP_LDS];               // part B's bucket counters
    __shared__ unsigned long long s_red[8];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_bad[4];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if ((int)blockIdx.x < groups4) {
        // part A: workgroup g takes bins 4 g .. 4 g + 3, one per wave, if they hold at most 256 entries
        const int bin = (int)blockIdx.x * 4 + w;
        const uint32_t n = bin < bins ? bin_total[bin] : 0u;
        const uint32_t start = bin < bins ? bin_start[bin] : 0u;     // asked for with the count, not after it: one round trip less
        if (n == 0 || n > (uint32_t)TSORT_LDS) return;
        unsigned long long* a = s_a + w * TSORT_LDS;
        // one wave, its own slice: LDS operations of a wave execute in order, so a wave-level fence is all the exchange
        // between its lanes needs (no workgroup barrier anywhere in this part)
        auto wsync = [] { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
                          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); };
        if (n <= (uint32_t)rank_max) {
            // the rank sort (rank_max: 0, 64, 128 or 256 -- launch_tile_binning): one or two words per lane up to 128 entries, four above
            // (n and start are the same in every lane: say so, the walk's loop then runs on the scalar unit)
            const uint32_t un = (uint32_t)__builtin_amdgcn_readfirstlane((int)n), ustart = (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
            const unsigned long long* src = words + ustart;
            if (un <= 64u) rank_sort_wave<1>(src, un, a, ustart, bin, sub_shift, slot_bits, num_tiles, (uint32_t)l, point_list, ranges, inst_gid, list_gid, wsync);
            else if (un <= 128u) rank_sort_wave<2>(src, un, a, ustart, bin, sub_shift, slot_bits, num_tiles, (uint32_t)l, point_list, ranges, inst_gid, list_gid, wsync);
            else rank_sort_wave<4>(src, un, a, ustart, bin, sub_shift, slot_bits, num_tiles, (uint32_t)l, point_list, ranges, inst_gid, list_gid, wsync);
            return;
        }
        if (bucket_b == 2 && n > 64) {
            // the bucket sort by one wave in its own slices (C3: sort stage 19.4 -> 18.5 us, dense 1 M cloud 59.4 -> 56.2;
            // profiles/r04d_ab_tsort_wave.json)
            bucket_sort_bin<64, TSORT_LDS / 64>(words + start, n, slot_bits, a, s_cnt + w * TSORT_LDS, s_red + 2 * w, s_wave + w,
                                                &s_bad[w], l, wsync);
            write_sorted(a, n, start, bin, sub_shift, slot_bits, num_tiles, (uint32_t)l, 64u, point_list, ranges, inst_gid, list_gid);
            return;
        }
        for (uint32_t i = l; i < n; i += 64) a[i] = words[start + i];
        wsync();
        if (n > 1) bitonic_sort(a, n, (uint32_t)l, 64u, wsync);
        write_sorted(a, n, start, bin, sub_shift, slot_bits, num_tiles, (uint32_t)l, 64u, point_list, ranges, inst_gid, list_gid);
        return;
    }
    // part B: the remaining workgroups walk the bins with a stride and take those of 257..1024 entries, one at a time, with
    // the four slices as one array (a sparse view has none: these workgroups read their bins' counts and leave)
    const int first = (int)blockIdx.x - groups4, stride = (int)gridDim.x - groups4;
    for (int bin = first; bin < bins; bin += stride) {
        const uint32_t n = bin_total[bin];
        if (n <= (uint32_t)TSORT_LDS || n > (uint32_t)TSORT_GROUP_LDS) continue;
        const uint32_t start = bin_start[bin];
        lds_barrier();
        if (bucket_b) {
            // the bucket sort of k_tile_sort_large at this size: 4 entries and 4 buckets per thread, ~7 barriers instead of
            // the network's 45-55
            bucket_sort_bin<256, TSORT_GROUP_LDS / 256>(words + start, n, slot_bits, s_a, s_cnt, s_red, s_wave, &s_bad[0],
                                                        (int)threadIdx.x, [] { lds_barrier(); });
        } else {
            for (uint32_t i = threadIdx.x; i < n; i += 256) s_a[i] = words[start + i];
            lds_barrier();
            bitonic_sort(s_a, n, threadIdx.x, 256u, [] { lds_barrier(); });
        }
        write_sorted(s_a, n, start, bin, sub_shift, slot_bits, num_tiles, threadIdx.x, 256u, point_list, ranges, inst_gid, list_gid);
    }
