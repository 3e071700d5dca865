// loss_ssim_fwd_body.h -- the body of the L1 + DSSIM forward kernels k_ssim_fwd and k_ssim_fwd_masked (loss.hip), included
// INSIDE each of them with `MASKED` (constexpr bool) and `mask` in scope.  Textual inclusion, not an inlined __device__ function:
// the function form changed k_ssim_fwd's instruction stream, and the plain kernel must stay instruction for instruction what it
// was (as gauss_bwd_body.h).  MASKED: the pair is (m I, m G) for a content mask m [H,W] shared by the channels -- m is
// multiplied into both images as the halo is staged, and the rest of the pass is the plain one.
// NOT a stand-alone header (no include guard on purpose).
    // One LDS buffer, two tenants: the staged halo regions of I and G, then -- once every thread holds its horizontal
    // sums in registers -- the five horizontal maps.  28 KB instead of 42 KB per workgroup: 5 workgroups per CU, not 3
    // (the kernel is a chain of memory and LDS round trips; what it lacks is waves to hide them).
    __shared__ float s_raw[5 * LR_IN * (LT + 1)];
    float (*s_i)[LR_IN + 1] = reinterpret_cast<float (*)[LR_IN + 1]>(s_raw);
    float (*s_g)[LR_IN + 1] = reinterpret_cast<float (*)[LR_IN + 1]>(s_raw + LR_IN * (LR_IN + 1));
    float (*s_h)[LR_IN][LT + 1] = reinterpret_cast<float (*)[LR_IN][LT + 1]>(s_raw);     // I, G, I^2, G^2, I*G
    static_assert(2 * LR_IN * (LR_IN + 1) <= 5 * LR_IN * (LT + 1), "the halo regions must fit under the horizontal maps");
    __shared__ float s_tmp[4];

    const int lb = xcd_band_block(n_blocks);
    if (lb < 0) return;
    const int tile = lb % (tiles_x * tiles_y), ch = lb / (tiles_x * tiles_y);
    const int x0 = (tile % tiles_x) * LT, y0 = (tile / tiles_x) * LT;
    const size_t plane = (size_t)ch * H * W;
    const int tid = threadIdx.x;

    // stage the halo region: ALL global loads of the thread are issued before the first LDS store (the workgroup's run
    // time is a chain of memory round trips at 3-5 waves per SIMD; a rolled loop pays one round trip per iteration).
    // Element p = tid + 256 i of the 42x42 region: (row, column) advance by (6, 4) per step with one carry -- one
    // integer division per thread instead of two per element (index arithmetic was a third of the kernel's instructions).
    float l1_part = 0.f;
    {
        const float* __restrict__ ip = img + plane;
        const float* __restrict__ gp = gt + plane;
        float ra[NSTAGE], rb[NSTAGE];
        int li[NSTAGE];                                       // LDS index, -1: nothing to store
        bool inner[NSTAGE];
        int ly = tid / LR_IN, lx = tid - ly * LR_IN;
#pragma unroll
        for (int i = 0; i < NSTAGE; i++) {
            const int y = y0 + ly - HALO, x = x0 + lx - HALO;
            const bool in_region = tid + i * LTHREADS < LR_IN * LR_IN;
            const bool ok = in_region && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
            const int q = ok ? y * W + x : 0;
            const float a = ip[q], b = gp[q];
            if constexpr (MASKED) {
                const float mv = mask[q];
                ra[i] = ok ? a * mv : 0.f; rb[i] = ok ? b * mv : 0.f;
            } else {
                ra[i] = ok ? a : 0.f; rb[i] = ok ? b : 0.f;
            }
            li[i] = in_region ? ly * (LR_IN + 1) + lx : -1;
            inner[i] = in_region && (unsigned)(ly - HALO) < (unsigned)LT && (unsigned)(lx - HALO) < (unsigned)LT;
            lx += LTHREADS % LR_IN; ly += LTHREADS / LR_IN;
            if (lx >= LR_IN) { lx -= LR_IN; ly += 1; }
        }
#pragma unroll
        for (int i = 0; i < NSTAGE; i++) {
            if (li[i] >= 0) {
                (&s_i[0][0])[li[i]] = ra[i]; (&s_g[0][0])[li[i]] = rb[i];
                if (inner[i]) l1_part += fabsf(ra[i] - rb[i]);                          // outside the image = 0
            }
        }
    }
    lds_barrier();

    // horizontal pass: item = (row, group of 4 adjacent output columns); 336 items = up to two per thread, kept in
    // registers until every thread has read its inputs (the maps overwrite the halo regions)
    constexpr int HITEMS = LR_IN * (LT / 4), HROUNDS = (HITEMS + LTHREADS - 1) / LTHREADS;
    float hs[HROUNDS][5][4];
#pragma unroll
    for (int r = 0; r < HROUNDS; r++) {
        const int it = tid + r * LTHREADS;
        if (it < HITEMS) {
            const int row = it / (LT / 4), c0 = (it % (LT / 4)) * 4;
            float a[14], b[14];
#pragma unroll
            for (int k = 0; k < 14; k++) { a[k] = s_i[row][c0 + k]; b[k] = s_g[row][c0 + k]; }
#pragma unroll
            for (int o = 0; o < 4; o++) {
                float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
                for (int k = 0; k < 11; k++) {
                    const float w = win.w[k], u = a[o + k], v = b[o + k];
                    m1 += w * u; m2 += w * v; e11 += w * (u * u); e22 += w * (v * v); e12 += w * (u * v);
                }
                hs[r][0][o] = m1; hs[r][1][o] = m2; hs[r][2][o] = e11; hs[r][3][o] = e22; hs[r][4][o] = e12;
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
            for (int m = 0; m < 5; m++)
#pragma unroll
                for (int o = 0; o < 4; o++) s_h[m][row][c0 + o] = hs[r][m][o];
        }
    }
    lds_barrier();

    // vertical pass: thread = (column, group of 4 adjacent output rows)
    const int col = tid % LT, r0 = (tid / LT) * 4;
    float acc[5][4];
#pragma unroll
    for (int m = 0; m < 5; m++) {
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
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    float ssim_part = 0.f;
    float* __restrict__ d1p = D1 + plane;
    float* __restrict__ d2p = D2 + plane;
    float* __restrict__ d3p = D3 + plane;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const int y = y0 + r0 + o, x = x0 + col;
        if (y < H && x < W) {
            const float mu1 = acc[0][o], mu2 = acc[1][o];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = acc[2][o] - mu1_sq, s2 = acc[3][o] - mu2_sq, s12 = acc[4][o] - mu12;
            const float A1 = 2.f * mu12 + C1, A2 = 2.f * s12 + C2, B1 = mu1_sq + mu2_sq + C1, B2 = s1 + s2 + C2;
            // two v_rcp_f32 (1 ulp) instead of three IEEE divisions: B1 >= C1, B2 >= C2 up to rounding, no special cases
            const float iB1 = __builtin_amdgcn_rcpf(B1), iB2 = __builtin_amdgcn_rcpf(B2);
            const float inv = iB1 * iB2;
            const float S = A1 * A2 * inv;
            ssim_part += S;
            // partial derivatives of S w.r.t. the window sums of I, I^2 and I*G (those of G, G^2 are not needed)
            const float dA1 = A2 * inv, dA2 = A1 * inv, dB1 = -S * iB1, dB2 = -S * iB2;
            const int q = y * W + x;
            d1p[q] = dA1 * 2.f * mu2 + dB1 * 2.f * mu1 - dB2 * 2.f * mu1 - dA2 * 2.f * mu2;
            d2p[q] = dB2;
            d3p[q] = 2.f * dA2;
        }
    }
    const float st = block_sum(ssim_part, s_tmp);
    const float lt = block_sum(l1_part, s_tmp);
    if (tid == 0) partials[lb] = make_float2(st, lt);
