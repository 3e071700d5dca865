// render_bwd_tile_body.h -- the body of the one-wave-per-tile blend backward (render_bwd.hip render_bwd_tile, where the design is
// described), included INSIDE a function that has its parameters (tile, seg, ck_slot, c_final, W, H, gx, ranges, point_list, rec, bg,
// final_Ts, n_contrib, dL_dpix, bin_base, hdr, dL_dalpha), the constants BATCH, STRICT, LDSRED, ALPHA, HAND and LANE_AGAIN, and the LDS arrays
// s_q0, s_q1, s_q2 [BATCH] float4, s_id [BATCH], s_acc [BATCH * 12] and s_tr (lds_reduce9's planes, 256-byte aligned) in scope.
// HAND (k_render_bwd_tile_step): a pixel's final T and stop position come from the forward half's registers, hand_T[q] and
// hand_last[q] (render_fwd_tile_body.h), instead of final_Ts / n_contrib.
    const int tx = tile % gx, ty = tile / gx;
    // (LANE_AGAIN, k_render_bwd_tile_step: the lane's index is formed again from the hardware's lane count, behind something the
    // optimiser cannot see through -- not a register kept across the forward half, and in the segment loop what is derived from it
    // is formed inside the loop, not kept across it; the wave is whole here)
    int l_src = threadIdx.x;
    if constexpr (LANE_AGAIN) {
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l_src));
    }
    const int l = l_src;
    const int x0 = tx * TILE_X, y0 = ty * TILE_Y;
    const int pxL = x0 + (l & 7), pxR = pxL + 8, pyT = y0 + (l >> 3), pyB = pyT + 8;
    const float pyTf = (float)pyT, pyBf = (float)pyB;
    const size_t N = (size_t)W * H;

    const uint2 range = ranges[tile];
    const int total = (int)(range.y - range.x);
    if (total == 0) return;
    const int seg_lo = seg < 0 ? 0 : seg * BWD_SEG;                    // as render_bwd_item
    const int seg_hi = seg < 0 ? total : min(total, seg_lo + BWD_SEG);
    if (seg_lo >= seg_hi) return;
    const BinLayout BL = bin_layout((long long)hdr->bin_bound);
    const uint32_t* __restrict__ list_gid = reinterpret_cast<const uint32_t*>(bin_base + BL.list_gid);
    float4* __restrict__ inst_grad = reinterpret_cast<float4*>(bin_base + BL.inst_grad);
    const uint32_t* __restrict__ quad_hits = reinterpret_cast<const uint32_t*>(bin_base + BL.quad_hits);
    const float4* __restrict__ ck = reinterpret_cast<const float4*>(bin_base + BL.ckpt) + (size_t)ck_slot * TILE_PIX;

    // quadrant q = x half + 2 * y half (the forward's wave q): P0 upper left, P1 upper right, P2 lower left, P3 lower right
    BwdPix P0, P1, P2, P3;
    const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
    auto load_pixel = [&](BwdPix& p, int px, int py, int q) {
        const bool ins = px < W && py < H;
        const size_t pix = (size_t)py * W + px;
        p.pxf = (float)px;
        if constexpr (HAND) { p.T = hand_T[q]; p.last = hand_last[q]; }
        else {
            p.T = ins ? final_Ts[pix] : 0.f;
            p.last = ins ? n_contrib[pix] : 0u;
        }
        p.dLr = ins ? dL_dpix[pix] : 0.f;
        p.dLg = ins ? dL_dpix[N + pix] : 0.f;
        p.dLb = ins ? dL_dpix[2 * N + pix] : 0.f;
        p.A = bg0 * p.dLr + bg1 * p.dLg + bg2 * p.dLb;
        float ga = 0.f;
        if constexpr (ALPHA) {
            ga = ins ? dL_dalpha[pix] : 0.f;
            p.A -= ga;
        }
        if (seg_hi < total && p.last > (uint32_t)seg_hi) {          // as render_bwd_item: the forward's state at the segment's deep end
            const float4 c = ck[q * 64 + l], f = c_final[pix];
            if constexpr (ALPHA)
                p.A = ((f.x - c.y) * p.dLr + (f.y - c.z) * p.dLg + (f.z - c.w) * p.dLb - ga * p.T) * __builtin_amdgcn_rcpf(c.x);
            p.T = c.x;
            if constexpr (!ALPHA)
                p.A = ((f.x - c.y) * p.dLr + (f.y - c.z) * p.dLg + (f.z - c.w) * p.dLb) * __builtin_amdgcn_rcpf(c.x);
        }
    };
    load_pixel(P0, pxL, pyT, 0); load_pixel(P1, pxR, pyT, 1); load_pixel(P2, pxL, pyB, 2); load_pixel(P3, pxR, pyB, 3);
    const uint32_t last0 = wave_max_u32(P0.last), last1 = wave_max_u32(P1.last);
    const uint32_t last2 = wave_max_u32(P2.last), last3 = wave_max_u32(P3.last);
    const uint32_t tile_last = max(max(last0, last1), max(last2, last3));

    const int row = l >> 4;
    const int col_a = (row == 0) ? 0 : (row == 1) ? 2 : (row == 2) ? 1 : 3;     // as k_render_bwd (reduce8 / row_merge3 layout)
    const int l16 = l & 15;
    const bool merge_writer = (l16 & 3) == 0 && l16 < 12;
    // lds_reduce9 leaves terms 2 row / 2 row + 1 in lanes 0 / 8 (term t IS column t) and the row's db partial in lane 4
    const int merge_off = LDSRED ? (l16 == 0 ? 2 * row : l16 == 8 ? 2 * row + 1 : 8 + row)
                                 : (l16 == 0 ? col_a : l16 == 8 ? col_a + 4 : 8 + row);
    uint32_t tr_base = 0u, tr_a1 = 0u;
    if (LDSRED) {
        tr_base = (uint32_t)(uintptr_t)s_tr;
        const int t = l >> 3, sh = (l >> 2) & 1;
        tr_a1 = tr_base + (uint32_t)(t * 256 + (((t & 3) < 2) ? sh : 3 - sh) * 64 + (l & 3) * 16);
    }

    for (int base = 0; base < seg_hi - seg_lo; base += BATCH) {
        const int cnt = min(BATCH, seg_hi - seg_lo - base);
        const int pos_hi = seg_hi - 1 - base;            // position of staged element 0 (back to front)
        const int pos_lo = pos_hi - (cnt - 1);
        if ((uint32_t)pos_lo >= tile_last) {             // whole batch behind every last contributor: slots read as zero
            int lz = l;
            if constexpr (LANE_AGAIN) asm volatile("" : "+v"(lz));          // (as lv below: `seg_hi - 1 - l` is not kept across the rounds)
            if (lz < cnt) {
                float4* slot = inst_grad + 3 * (size_t)point_list[range.x + (pos_hi - lz)];
                slot[0] = make_float4(0.f, 0.f, 0.f, 0.f); slot[1] = slot[0]; slot[2] = slot[0];
            }
            continue;
        }
        lds_barrier();
        // the lane's staging / flush addresses are formed HERE, per round, from a lane index the optimiser cannot see through:
        // hoisted out of the loop they are seven more live registers in a kernel that has 64, i.e. seven spilled dwords per
        // lane (15 MB of scratch stores per 1080p view, round 6) for a handful of integer operations per round
        int lv = l;
        asm volatile("" : "+v"(lv));
        uint32_t my_hit = 0u;
        if (lv < cnt) {
            const uint32_t e = point_list[range.x + (pos_hi - lv)];
            my_hit = quad_hits[range.x + (pos_hi - lv)];
            const uint32_t id = list_gid[range.x + (pos_hi - lv)];       // (BinLayout::list_gid: no gather through e)
            const float4* g = reinterpret_cast<const float4*>(rec + id);
            const float4 a = g[0], b = g[1], c = g[2];
            s_q0[lv] = STRICT ? make_float4(a.x, a.y, a.z, a.w) : make_float4(a.x, a.y, (-0.5f * LOG2E) * a.z, -LOG2E * a.w);
            *reinterpret_cast<float2*>(&s_q1[lv]) = STRICT ? make_float2(b.x, b.y) : make_float2((-0.5f * LOG2E) * b.x, b.y);
            s_q2[lv] = make_float4(b.z, b.w, c.x, 0.f);
            s_id[lv] = e;
        }
        if (lv < BATCH) {
            float4* z = reinterpret_cast<float4*>(&s_acc[lv * 12]);
            z[0] = make_float4(0.f, 0.f, 0.f, 0.f); z[1] = z[0]; z[2] = z[0];
        }
        lds_barrier();

        // CULL: the staging lane IS the lane that holds the element's quadrant tests (one batch = one wave-wide chunk)
        const int lc = LANE_AGAIN ? lv : l;                                 // (as lz above)
        const uint32_t pos_l = (uint32_t)(pos_hi - lc);
        const bool inb = lc < cnt;
        const uint64_t m0 = __ballot(inb && pos_l < last0 && (my_hit & 0x000000ffu) != 0u);
        const uint64_t m1 = __ballot(inb && pos_l < last1 && (my_hit & 0x0000ff00u) != 0u);
        const uint64_t m2 = __ballot(inb && pos_l < last2 && (my_hit & 0x00ff0000u) != 0u);
        const uint64_t m3 = __ballot(inb && pos_l < last3 && (my_hit & 0xff000000u) != 0u);
        uint64_t mask = (m0 | m1) | (m2 | m3);
        // (always the copy WITH the `pos < last` test: a second copy of this loop costs the 64-VGPR budget 28 more spilled bytes
        //  and the kernel 5 % -- measured 96.0 -> 101.0 us at C3, profiles/r04i_ab_bwd_nocheck_tile.json)
        constexpr bool CHECK = true;
        while (mask) {
            const int j = __ffsll((long long)mask) - 1;       // staged order is already back to front
            mask &= mask - 1;
            const uint32_t pos = (uint32_t)(pos_hi - j);
            const float4 a = s_q0[j];
            const float2 b = *reinterpret_cast<const float2*>(&s_q1[j]);   // Cp, opacity
            const float4 c = s_q2[j];
            const float dysT = a.y - pyTf, dysB = a.y - pyBf;
            float tD = 0.f, tMx = 0.f, tMxx = 0.f, bD = 0.f, bMx = 0.f, bMxx = 0.f, sR = 0.f, sG = 0.f, sB = 0.f;
            const bool h0 = (m0 >> j) & 1ull, h1 = (m1 >> j) & 1ull, h2 = (m2 >> j) & 1ull, h3 = (m3 >> j) & 1ull;
            if (h0 || h1) {
                float Bd, Cdd;
                gauss_row<STRICT>(a.w, b.x, dysT, Bd, Cdd);                                              // common.h gauss_power
                if (h0) bwd_pixel<true, true, CHECK, STRICT>(P0, a.z, a.w, b.x, Bd, Cdd, a.x, b.y, c.x, c.y, c.z, pos, tD, tMx, tMxx, sR, sG, sB);
                if (h1) bwd_pixel<false, false, CHECK, STRICT>(P1, a.z, a.w, b.x, Bd, Cdd, a.x, b.y, c.x, c.y, c.z, pos, tD, tMx, tMxx, sR, sG, sB);
            }
            if (h2 || h3) {
                float Bd, Cdd;
                gauss_row<STRICT>(a.w, b.x, dysB, Bd, Cdd);
                if (h2) bwd_pixel<true, false, CHECK, STRICT>(P2, a.z, a.w, b.x, Bd, Cdd, a.x, b.y, c.x, c.y, c.z, pos, bD, bMx, bMxx, sR, sG, sB);
                if (h3) bwd_pixel<false, false, CHECK, STRICT>(P3, a.z, a.w, b.x, Bd, Cdd, a.x, b.y, c.x, c.y, c.z, pos, bD, bMx, bMxx, sR, sG, sB);
            }
            // the dy factors, per pixel pair (a pair shares its row)
            const float t1 = dysT * tD, t2 = dysB * bD;
            const float sD = tD + bD, sMxx = tMxx + bMxx;
            const float sMy = t1 + t2;
            const float sMxy = dysT * tMx + dysB * bMx;
            const float sMyy = dysT * t1 + dysB * t2;
            float rc;
            if (LDSRED) {
                rc = lds_reduce9(tMx + bMx, sMy, sMxx, sMxy, sMyy, sD, sR, sG, sB, tr_base, tr_a1, tr_a1 ^ 128u);
            } else {
                float ra = tMx + bMx;
                float rb = sMyy;
                reduce8(ra, sMy, sMxx, sMxy, rb, sD, sR, sG);
                rc = row_merge3(ra, rb, sB);
            }
            int jo = j * 12;
            asm volatile("" : "+s"(jo));                      // scalar product, one v_add for the address (not a v_mad_u64_u32)
            if (merge_writer) s_acc[jo + merge_off] = rc;
        }
        lds_barrier();
        if (lv < cnt) {
            int Wv = W, Hv = H;
            asm volatile("" : "+s"(Wv), "+s"(Hv));               // (as lv: formed per round, not kept in two registers)
            const float ddelx_dx = (float)(0.5 * Wv);            // backward.cu:473-474 (double product, rounded once)
            const float ddely_dy = (float)(0.5 * Hv);
            float a9[12];
#pragma unroll
            for (int k = 0; k < 12; k++) a9[k] = s_acc[lv * 12 + k];
            const float4 q0 = s_q0[lv]; const float2 q1 = *reinterpret_cast<const float2*>(&s_q1[lv]);
            const float db = (a9[8] + a9[9]) + (a9[10] + a9[11]);
            const float ca = STRICT ? q0.z : (-2.0f * LN2) * q0.z, cb = STRICT ? q0.w : -LN2 * q0.w,
                        cc = STRICT ? q1.x : (-2.0f * LN2) * q1.x, o = q1.y;
            const float sx = a9[0], sy = a9[1], h = -0.5f;          // as k_render_bwd: the sums carry the opacity factor
            const float dopac = o > 0.f ? a9[5] * __builtin_amdgcn_rcpf(o) : 0.f;      // 1 ulp: the sum itself carries more
            float4* slot = inst_grad + 3 * (size_t)s_id[lv];
            slot[0] = make_float4((-ca * sx - cb * sy) * ddelx_dx, (-cc * sy - cb * sx) * ddely_dy, h * a9[2], h * a9[3]);
            slot[1] = make_float4(h * a9[4], dopac, a9[6], a9[7]);
            slot[2] = make_float4(db, 0.f, 0.f, 0.f);
        }
    }
