// gauss_bwd_body.h -- the body of the per-Gaussian backward kernels k_gauss_bwd and k_gauss_bwd_depth (gauss_bwd.hip),
// included INSIDE each of them with `RAW`, `AA` (template parameters) and `DEPTH` (constexpr bool) in scope.  Textual inclusion, not an
// inlined __device__ function: the function form changed k_gauss_bwd's instruction stream (operand order of its slot sums), and
// the default kernel must stay instruction for instruction what it was.  DEPTH: the slots' dL/d(view depth) float is summed too.
// ABSG (k_gauss_bwd_abs; constexpr bool, with `dL_dmean2D_abs` in scope): the slots' two absgrad floats (g2.z, g2.w: the blend
// backward's sums of |per-pixel dL/dmean2D|) are summed too and written -- never accumulated -- to dL_dmean2D_abs [P,3] as {x, y, 0}.
// AA && !RAW: the record's opacity (opacity * coef, what the blend saw) is read from the geom buffer, whose first bytes are `hdr`.
// STATS (k_gauss_bwd_stats; constexpr bool, with `stat_accum` in scope): the norm of the view's own dL/dmean2D -- with ABSG of the two
// absgrad sums instead, which are then NOT written to dL_dmean2D_abs -- is handed to gauss_backward_one<STATS>, which accumulates it.
// NOT a stand-alone header (no include guard on purpose).
    constexpr uint32_t SERIAL_MAX = 24;      // instances summed by the owning lane; more -> whole wave helps
    constexpr int BST = 17;                  // LDS row stride (floats) of the per-Gaussian basis rows: odd -> no conflicts
    __shared__ uint32_t s_idx[GB_THREADS];
    __shared__ float s_b[4][32 * BST];           // basis, d/dx, d/dy, d/dz of 32 Gaussians (half a round)
    __shared__ float s_rgb[3][GB_THREADS];       // dL/dRGB after the clamp mask
    __shared__ float s_ddir[3][GB_THREADS];      // dL/d(view direction)
    const int lane = threadIdx.x;
    const uint32_t n = hdr->num_compact;
    if (n == 0) return;
    if (hdr->overflow != 0u) return;         // async mode: an overflowed view contributes nothing (see k_render_bwd)
    // per-instance partial sums written by k_render_bwd (48-byte slots, contiguous per Gaussian in emission
    // order); slots at or beyond num_sorted were never built (async-mode overflow) and are ignored
    const float4* __restrict__ inst_grad =
        reinterpret_cast<const float4*>(bin_base + bin_layout((long long)hdr->bin_bound).inst_grad);
    const uint32_t n_slots = hdr->num_sorted;

    for (uint32_t t0 = blockIdx.x * GB_THREADS; t0 < n; t0 += gridDim.x * GB_THREADS) {
        const uint32_t t = t0 + threadIdx.x;
        const bool live = t < n;
        const int idx = live ? (int)vis_list[t] : 0;
        s_idx[lane] = (uint32_t)idx;
        float rec_opacity = 0.f;
        if constexpr (AA && !RAW) {
            // geom_layout (common.h): the records follow the 256-byte header
            const GaussRec* __restrict__ rec = reinterpret_cast<const GaussRec*>(reinterpret_cast<const char*>(hdr) + align_up(sizeof(GeomHeader)));
            if (live) rec_opacity = rec[idx].opacity;
        }
        // first instance slot and instance count from the rank-ordered `offsets` (dense reads: neighbouring lanes read
        // neighbouring words) instead of goff[idx] / tiles_touched[idx] -- two more 64-byte lines per visible Gaussian for
        // 4 useful bytes each when ~9 % of the Gaussians are visible
        const uint32_t off = live ? offsets[t] : 0u;
        const uint32_t tt = live ? ((t + 1 < n) ? offsets[t + 1] : hdr->num_instances) - off : 0u;
        float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0, g2 = g0;
        if (tt <= SERIAL_MAX && off < n_slots) {
            // four slots per step with independent loads (a one-slot loop pays one memory latency per instance)
            const uint32_t cnt = min(tt, n_slots - off);
            const float4* first = inst_grad + 3 * (size_t)off;
            for (uint32_t j = 0; j < cnt; j += 4) {
                float4 a[4][3];
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    const float4* slot = first + 3 * (size_t)min(j + q, cnt - 1);
                    a[q][0] = slot[0]; a[q][1] = slot[1]; a[q][2] = slot[2];
                }
#pragma unroll
                for (uint32_t q = 0; q < 4; q++)
                    if (j + q < cnt) { add4(g0, a[q][0]); add4(g1, a[q][1]); add4(g2, a[q][2]); }
            }
        }
        uint64_t big = __ballot(tt > SERIAL_MAX);
        while (big) {
            const int src = __ffsll((long long)big) - 1;
            big &= big - 1;
            const uint32_t b_tt = __shfl(tt, src), b_off = __shfl(off, src);
            float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
            for (uint32_t j = lane; j < b_tt; j += 64) {
                if (b_off + j >= n_slots) break;
                const float4* slot = inst_grad + 3 * (size_t)(b_off + j);
                add4(p0, slot[0]); add4(p1, slot[1]); add4(p2, slot[2]);
            }
            p0.x = wave_sum(p0.x); p0.y = wave_sum(p0.y); p0.z = wave_sum(p0.z); p0.w = wave_sum(p0.w);
            p1.x = wave_sum(p1.x); p1.y = wave_sum(p1.y); p1.z = wave_sum(p1.z); p1.w = wave_sum(p1.w);
            p2.x = wave_sum(p2.x);
            if constexpr (DEPTH) p2.y = wave_sum(p2.y);
            if constexpr (ABSG) { p2.z = wave_sum(p2.z); p2.w = wave_sum(p2.w); }
            if (lane == src) { g0 = p0; g1 = p1; g2 = p2; }
        }
        // ---- spherical harmonics: rows are 3*M floats per Gaussian.  One lane per Gaussian would make every
        // load/store instruction touch 64 different rows (64 cache lines for 16 useful bytes each, and the working
        // set of a wave overflows the L1); instead each lane computes the 16 basis values and their direction
        // derivatives of ITS Gaussian into LDS, and then 16 LANES share one Gaussian, lane k owning coefficient k:
        // a wave reads/updates 4 complete rows per step with fully used cache lines.
        V3 dL_ddir = { 0.f, 0.f, 0.f };
        const bool have_sh = shs != nullptr && dL_dsh != nullptr;
        if (have_sh) {
            const int k = lane & 15, sub = lane >> 4;
            const int K = (vp.D + 1) * (vp.D + 1);
            const size_t shrow = (size_t)vp.M * 3;
            const bool acc = (accum_mask >> ACC_SH) & 1u;
            const bool no_fill = !acc && (accum_mask >> 31) != 0u;          // LR_ACC_NO_ZERO_FILL (lucid_raster.h)
            const int n_here = (int)min((uint32_t)GB_THREADS, n - t0);
            if (live) {
                const uint8_t cb = clamped[idx];
                s_rgb[0][lane] = (cb & 1) ? 0.f : g1.z;
                s_rgb[1][lane] = (cb & 2) ? 0.f : g1.w;
                s_rgb[2][lane] = (cb & 4) ? 0.f : g2.x;
            }
            // two half rounds of 32 Gaussians keep the LDS footprint (and with it the occupancy limit) small
            for (int half = 0; half < 2; half++) {
                if (half * 32 >= n_here) break;
                if (live && (lane >> 5) == half) {
                    const size_t i = (size_t)idx;
                    const V3 d0 = { means3D[3 * i] - vp.campos[0], means3D[3 * i + 1] - vp.campos[1], means3D[3 * i + 2] - vp.campos[2] };
                    const float len = sqrtf(dot(d0, d0));
                    const V3 dir = { d0.x / len, d0.y / len, d0.z / len };
                    float b[16], bx[16], by[16], bz[16];
                    switch (vp.D) {
                        case 0: sh_basis<0>(dir, b, bx, by, bz); break;
                        case 1: sh_basis<1>(dir, b, bx, by, bz); break;
                        case 2: sh_basis<2>(dir, b, bx, by, bz); break;
                        default: sh_basis<3>(dir, b, bx, by, bz); break;
                    }
                    const int o = (lane & 31) * BST;
#pragma unroll
                    for (int q = 0; q < 16; q++) {
                        s_b[0][o + q] = b[q]; s_b[1][o + q] = bx[q]; s_b[2][o + q] = by[q]; s_b[3][o + q] = bz[q];
                    }
                }
                lds_barrier();
                // four steps (16 Gaussians) at a time: all row loads are issued before the first store, which the
                // compiler cannot do across steps by itself (the accumulate loads may alias the previous stores)
                for (int it0 = 0; it0 < 8; it0 += 4) {
                    if (half * 32 + it0 * 4 >= n_here) break;
                    float sv[4][3], dv[4][3];
                    size_t rowv[4];
                    bool onv[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int gl = (it0 + q) * 4 + sub, g = half * 32 + gl;
                        onv[q] = g < n_here && k < K;
                        const size_t gi = (size_t)s_idx[onv[q] ? g : 0];
                        const int kk = onv[q] ? k : 0;
                        // raw mode: coefficient 0 lives in features_dc [P,3], the others in features_rest [P,M-1,3]
                        rowv[q] = !RAW ? gi * shrow + 3 * kk : (kk == 0 ? gi * 3 : gi * (shrow - 3) + 3 * (kk - 1));
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const bool in_rest = RAW && onv[q] && k != 0;      // idle lanes re-read row 0 of features_dc
                        const float* sp = (in_rest ? vp.sh_rest : shs) + rowv[q];
                        sv[q][0] = sp[0]; sv[q][1] = sp[1]; sv[q][2] = sp[2];
                        if (acc) { const float* dp = (in_rest ? vp.dL_dsh_rest : dL_dsh) + rowv[q]; dv[q][0] = dp[0]; dv[q][1] = dp[1]; dv[q][2] = dp[2]; }
                        else { dv[q][0] = 0.f; dv[q][1] = 0.f; dv[q][2] = 0.f; }
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int gl = (it0 + q) * 4 + sub, g = half * 32 + gl;
                        const int gs = onv[q] ? g : 0, gls = onv[q] ? gl : 0, ks = onv[q] ? k : 0;
                        const float r0 = s_rgb[0][gs], r1 = s_rgb[1][gs], r2 = s_rgb[2][gs];
                        const float bk = s_b[0][gls * BST + ks];
                        if (onv[q]) {
                            float* dp = ((RAW && k != 0) ? vp.dL_dsh_rest : dL_dsh) + rowv[q];   // onv[q] holds here
                            dp[0] = dv[q][0] + bk * r0; dp[1] = dv[q][1] + bk * r1; dp[2] = dv[q][2] + bk * r2;
                        } else if (no_fill && g < n_here && k >= K && k < vp.M) {
                            // LR_ACC_NO_ZERO_FILL: nobody zero-filled the tensor, and a VISITED Gaussian's rows are read by the
                            // masked optimizer step -- its coefficients above the active degree are written as the zeros they are
                            const size_t gi = (size_t)s_idx[g];
                            float* dp = !RAW ? dL_dsh + gi * shrow + 3 * k
                                             : (k == 0 ? dL_dsh + gi * 3 : vp.dL_dsh_rest + gi * (shrow - 3) + 3 * (size_t)(k - 1));
                            dp[0] = 0.f; dp[1] = 0.f; dp[2] = 0.f;
                        }
                        const float sd = onv[q] ? sv[q][0] * r0 + sv[q][1] * r1 + sv[q][2] * r2 : 0.f;
                        const float px = row_sum(s_b[1][gls * BST + ks] * sd);
                        const float py = row_sum(s_b[2][gls * BST + ks] * sd);
                        const float pz = row_sum(s_b[3][gls * BST + ks] * sd);
                        if (k == 0 && g < n_here) { s_ddir[0][g] = px; s_ddir[1][g] = py; s_ddir[2][g] = pz; }
                    }
                }
                lds_barrier();
            }
            if (live) dL_ddir = { s_ddir[0][lane], s_ddir[1][lane], s_ddir[2][lane] };
        }
        float stat_norm = 0.f;
        if constexpr (STATS) stat_norm = ABSG ? sqrtf(g2.z * g2.z + g2.w * g2.w) : sqrtf(g0.x * g0.x + g0.y * g0.y);
        if (live)
            gauss_backward_one<RAW, DEPTH, AA, STATS>(idx, vp, means3D, scales, rotations, have_sh, dL_ddir, cov3D_precomp, g0, g1, g2,
                               dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dscale,
                               dL_drot, accum_mask, acc16, rec_opacity, stat_norm, stat_accum);
        if constexpr (ABSG && !STATS) {
            if (live) {
                float* __restrict__ pa = dL_dmean2D_abs + 3 * (size_t)idx;
                pa[0] = g2.z; pa[1] = g2.w; pa[2] = 0.f;
            }
        }
        lds_barrier();                     // the LDS planes are rewritten by the next round
    }
