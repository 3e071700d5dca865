// loss_ssim_bwd_body.h -- the body of the L1 + DSSIM backward kernels k_ssim_bwd and k_ssim_bwd_masked (loss.hip), included
// INSIDE each of them with `MASKED` (constexpr bool) and `mask` in scope (see loss_ssim_fwd_body.h for why it is textual).
// MASKED: I, G at q are the masked m I, m G of the forward, and dL/dI(q) = m(q) dL/d(m I)(q).
// NOT a stand-alone header (no include guard on purpose).
    // as in k_ssim_fwd: the three horizontal maps take over the LDS of the staged halo regions (22 KB instead of 38 KB)
    __shared__ float s_raw[3 * LR_IN * (LR_IN + 1)];
    static_assert(sizeof(float) * 3 * LR_IN * (LR_IN + 1) >= sizeof(double) * 2 * LTHREADS, "scratch of the final sum");
    // fused step (views_core): the loss value's final sum rides in workgroup 0 instead of a launch of its own
    if (out3 != nullptr && blockIdx.x == 0) {
        double* s_a = reinterpret_cast<double*>(s_raw);
        loss_final(n_blocks, n_elems, lambda, partials, out3, s_a, s_a + LTHREADS);
        lds_barrier();
    }
    float (*s_d)[LR_IN][LR_IN + 1] = reinterpret_cast<float (*)[LR_IN][LR_IN + 1]>(s_raw);
    float (*s_h)[LR_IN][LT + 1] = reinterpret_cast<float (*)[LR_IN][LT + 1]>(s_raw);
    const int lb = xcd_band_block(n_blocks);
    if (lb < 0) return;
    const int tile = lb % (tiles_x * tiles_y), ch = lb / (tiles_x * tiles_y);
    const int x0 = (tile % tiles_x) * LT, y0 = (tile / tiles_x) * LT;
    const size_t plane = (size_t)ch * H * W;
    const int tid = threadIdx.x;

    // the pixel's own I and G (needed only in the last lines) are requested first, together with the halo loads: as the
    // kernel's final dependent loads they cost every workgroup one more memory round trip
    const int col = tid % LT, r0 = (tid / LT) * 4;
    const float* __restrict__ ip = img + plane;
    const float* __restrict__ gp = gt + plane;
    float own_i[4], own_g[4], own_m[4];
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const int y = y0 + r0 + o, x = x0 + col;
        const int q = (y < H && x < W) ? y * W + x : 0;
        own_i[o] = ip[q]; own_g[o] = gp[q];
        if constexpr (MASKED) own_m[o] = mask[q];
    }
    {
        const float* __restrict__ p1 = D1 + plane;
        const float* __restrict__ p2 = D2 + plane;
        const float* __restrict__ p3 = D3 + plane;
        float r1[NSTAGE], r2[NSTAGE], r3[NSTAGE];
        int li[NSTAGE];
        int ly = tid / LR_IN, lx = tid - ly * LR_IN;           // element tid + 256 i: (row, column) += (6, 4) with carry
#pragma unroll
        for (int i = 0; i < NSTAGE; i++) {                   // all loads first (see k_ssim_fwd)
            const int y = y0 + ly - HALO, x = x0 + lx - HALO;
            const bool in_region = tid + i * LTHREADS < LR_IN * LR_IN;
            const bool ok = in_region && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
            const int q = ok ? y * W + x : 0;
            const float a = p1[q], b = p2[q], c = p3[q];
            r1[i] = ok ? a : 0.f; r2[i] = ok ? b : 0.f; r3[i] = ok ? c : 0.f;
            li[i] = in_region ? ly * (LR_IN + 1) + lx : -1;
            lx += LTHREADS % LR_IN; ly += LTHREADS / LR_IN;
            if (lx >= LR_IN) { lx -= LR_IN; ly += 1; }
        }
#pragma unroll
        for (int i = 0; i < NSTAGE; i++)
            if (li[i] >= 0) { (&s_d[0][0][0])[li[i]] = r1[i]; (&s_d[1][0][0])[li[i]] = r2[i]; (&s_d[2][0][0])[li[i]] = r3[i]; }
    }
    lds_barrier();
    constexpr int HITEMS = LR_IN * (LT / 4), HROUNDS = (HITEMS + LTHREADS - 1) / LTHREADS;
    float hs[HROUNDS][3][4];
#pragma unroll
    for (int r = 0; r < HROUNDS; r++) {
        const int it = tid + r * LTHREADS;
        if (it < HITEMS) {
            const int row = it / (LT / 4), c0 = (it % (LT / 4)) * 4;
#pragma unroll
            for (int m = 0; m < 3; m++) {
                float v[14];
#pragma unroll
                for (int k = 0; k < 14; k++) v[k] = s_d[m][row][c0 + k];
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    float sum = 0.f;
#pragma unroll
                    for (int k = 0; k < 11; k++) sum += win.w[k] * v[o + k];
                    hs[r][m][o] = sum;
                }
            }
        }
    }
    lds_barrier();
#pragma unroll
    for (int r = 0; r < HROUNDS; r++) {
        const int it = tid + r * LTHREADS;
        if (it < HITEMS) {
            const int row = it / (LT / 4), c0 = (it % (LT / 4)) * 4;
#pragma unroll
            for (int m = 0; m < 3; m++)
#pragma unroll
                for (int o = 0; o < 4; o++) s_h[m][row][c0 + o] = hs[r][m][o];
        }
    }
    lds_barrier();
    float acc[3][4];
#pragma unroll
    for (int m = 0; m < 3; m++) {
        float v[14];
#pragma unroll
        for (int k = 0; k < 14; k++) v[k] = s_h[m][r0 + k][col];
#pragma unroll
        for (int o = 0; o < 4; o++) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) s += win.w[k] * v[o + k];
            acc[m][o] = s;
        }
    }
    const float up = upstream != nullptr ? upstream[0] : 1.0f;
    // two-weight form (lr_l1_dssim_backward_weights): upstream = dL/d l1, w_ssim = dL/d ssim, both device scalars -- the
    // caller composed the two means itself, with whatever weights
    const float k_ssim = w_ssim != nullptr ? inv_n * w_ssim[0] : -lambda * inv_n * up;
    const float k_l1 = w_ssim != nullptr ? inv_n * up : (1.0f - lambda) * inv_n * up;
    float* __restrict__ gradp = grad + plane;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const int y = y0 + r0 + o, x = x0 + col;
        if (y < H && x < W) {
            const int q = y * W + x;
            if constexpr (MASKED) {
                const float m = own_m[o], a = own_i[o] * m, b = own_g[o] * m;
                const float d = a - b;
                const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                gradp[q] = m * (k_ssim * (acc[0][o] + 2.f * a * acc[1][o] + b * acc[2][o]) + k_l1 * sgn);
            } else {
                const float a = own_i[o], b = own_g[o];
                const float d = a - b;
                const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);      // torch.abs backward: sign, 0 at 0
                gradp[q] = k_ssim * (acc[0][o] + 2.f * a * acc[1][o] + b * acc[2][o]) + k_l1 * sgn;
            }
        }
    }
