// gauss_bwd.hip -- per-Gaussian backward stage for gfx950.
//
// Replaces computeCov2DCUDA (RAST/cuda_rasterizer/backward.cu:144-274) and the backward
// preprocessCUDA (:346-396) with its helpers computeColorFromSH (:20-139) and computeCov3D
// (:278-341) -- fused into ONE streaming pass: read the 48-byte GradRec produced by the blend
// backward, recompute the forward intermediates from the inputs (cheaper than storing cov3D /
// re-reading it: HBM-bound kernel).  Only visible Gaussians (radii > 0) do any work or touch memory.
// Two output modes per tensor (bit in `accum_mask`):
//   write      : rows of visible Gaussians are stored; the library zero-fills the tensor first with one
//                multi-segment kernel (k_zero_segments), so callers still never pre-zero anything
//                (the reference memsets 300 B/Gaussian per backward, rasterize_points.cu:154-162);
//   accumulate : rows of visible Gaussians are ADDED to what is already there and culled rows are not
//                touched at all -- this fuses autograd's `grad += new_grad` pass (another 3 x 236 B per
//                Gaussian per view of HBM traffic) into the kernel when several views are accumulated.
#include "common.h"
#include "dispatch_flags.h"
#include <algorithm>

namespace lr {

namespace {

// SH basis values and their derivatives w.r.t. the (normalised) view direction, band by band
// (the coefficients of backward.cu:20-139: dRGB/dx = sum_k dbx[k] * sh[k], dL/dsh[k] = b[k] * dL/dRGB).
template <int DEG>
__device__ __forceinline__ void sh_basis(V3 dir, float (&b)[16], float (&bx)[16], float (&by)[16], float (&bz)[16])
{
    const float x = dir.x, y = dir.y, z = dir.z;
#pragma unroll
    for (int k = 0; k < 16; k++) { b[k] = 0.f; bx[k] = 0.f; by[k] = 0.f; bz[k] = 0.f; }
    b[0] = SH_C0;
    if (DEG > 0) {
        b[1] = -SH_C1 * y; by[1] = -SH_C1;
        b[2] = SH_C1 * z;  bz[2] = SH_C1;
        b[3] = -SH_C1 * x; bx[3] = -SH_C1;
        if (DEG > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[4] = SH_C2[0] * xy;                    bx[4] = SH_C2[0] * y;        by[4] = SH_C2[0] * x;
            b[5] = SH_C2[1] * yz;                    by[5] = SH_C2[1] * z;        bz[5] = SH_C2[1] * y;
            b[6] = SH_C2[2] * (2.f * zz - xx - yy);  bx[6] = SH_C2[2] * 2.f * -x; by[6] = SH_C2[2] * 2.f * -y;
            bz[6] = SH_C2[2] * 2.f * 2.f * z;
            b[7] = SH_C2[3] * xz;                    bx[7] = SH_C2[3] * z;        bz[7] = SH_C2[3] * x;
            b[8] = SH_C2[4] * (xx - yy);             bx[8] = SH_C2[4] * 2.f * x;  by[8] = SH_C2[4] * 2.f * -y;
            if (DEG > 2) {
                b[9] = SH_C3[0] * y * (3.f * xx - yy);
                bx[9] = SH_C3[0] * 3.f * 2.f * xy;   by[9] = SH_C3[0] * 3.f * (xx - yy);
                b[10] = SH_C3[1] * xy * z;
                bx[10] = SH_C3[1] * yz;              by[10] = SH_C3[1] * xz;      bz[10] = SH_C3[1] * xy;
                b[11] = SH_C3[2] * y * (4.f * zz - xx - yy);
                bx[11] = SH_C3[2] * -2.f * xy;       by[11] = SH_C3[2] * (-3.f * yy + 4.f * zz - xx);
                bz[11] = SH_C3[2] * 4.f * 2.f * yz;
                b[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
                bx[12] = SH_C3[3] * -3.f * 2.f * xz; by[12] = SH_C3[3] * -3.f * 2.f * yz;
                bz[12] = SH_C3[3] * 3.f * (2.f * zz - xx - yy);
                b[13] = SH_C3[4] * x * (4.f * zz - xx - yy);
                bx[13] = SH_C3[4] * (-3.f * xx + 4.f * zz - yy); by[13] = SH_C3[4] * -2.f * xy;
                bz[13] = SH_C3[4] * 4.f * 2.f * xz;
                b[14] = SH_C3[5] * z * (xx - yy);
                bx[14] = SH_C3[5] * 2.f * xz;        by[14] = SH_C3[5] * -2.f * yz; bz[14] = SH_C3[5] * (xx - yy);
                b[15] = SH_C3[6] * x * (xx - 3.f * yy);
                bx[15] = SH_C3[6] * 3.f * (xx - yy); by[15] = SH_C3[6] * -3.f * 2.f * xy;
            }
        }
    }
}

template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// sum within each 16-lane row; every lane of the row ends with the row total
__device__ __forceinline__ float row_sum(float v)
{
    v += dpp<0xB1>(v);            // quad_perm [1,0,3,2]
    v += dpp<0x4E>(v);            // quad_perm [2,3,0,1]
    v += dpp<0x141>(v);           // row_half_mirror
    v += dpp<0x140>(v);           // row_mirror
    return v;
}

// Backward of ONE visible Gaussian, everything except the spherical-harmonics rows (those are handled 16 lanes per
// Gaussian by the caller, which passes the resulting dL/d(view direction) in `dL_ddir` when `have_sh`).
// RAW (lr_view_backward with raw = 1) is a template parameter, not a run-time branch: with `if (vp.raw)` blocks in this function
// ROCm 7.2 hipcc produced wrong dL/dcov3D in the NON-raw path (verified on hardware by removing either block).
// DEPTH (k_gauss_bwd_depth): g2.y is the Gaussian's dL/d(view depth) from the depth-mode blend backward; it reaches the mean
// through z = view[2] x + view[6] y + view[10] z + view[14] (column-major view matrix, auxiliary.h:58-66) -- in the raw path
// the same term is dL/dxyz.
// AA (the view's forward ran anti-aliased, gauss_project.h aa_coef): the record's opacity is opacity * coef(a0, b, c0), so g1.y is
// dL/d(record opacity): dL/dopacity = g coef, and dL/drho = g rec_opacity / (2 rho) above the floor reaches the 2D covariance
// next to the conic's terms.  rec_opacity: the record's opacity (non-raw: read from the geom buffer by the caller; raw: recomputed).
// STATS (k_gauss_bwd_stats: lr_views_accumulate with the stat_* members): stat_norm, the norm of THIS view's screen-space gradient
// (signed or absolute: the caller's choice), is summed as well -- into float 13 of the acc16 row, which travels with the row
// anyway, or without acc16 straight into stat_accum [P] (the caller's xyz_gradient_accum; views are chained, so no atomics).
template <bool RAW, bool DEPTH = false, bool AA = false, bool STATS = false>
__device__ __forceinline__ void
gauss_backward_one(const int idx, const ViewParams& vp, const float* __restrict__ means3D, const float* __restrict__ scales,
            const float* __restrict__ rotations, const bool have_sh, const V3 dL_ddir,
            const float* __restrict__ cov3D_precomp, const float4 g0, const float4 g1, const float4 g2,
            float* __restrict__ dL_dmean2D, float* __restrict__ dL_dconic, float* __restrict__ dL_dopacity,
            float* __restrict__ dL_dcolor, float* __restrict__ dL_dmean3D, float* __restrict__ dL_dcov3D,
            float* __restrict__ dL_dscale, float* __restrict__ dL_drot,
            uint32_t accum_mask, float* __restrict__ acc16, const float rec_opacity = 0.f, const float stat_norm = 0.f,
            float* __restrict__ stat_accum = nullptr)
{
    const size_t i = (size_t)idx;
    const float* __restrict__ V = vp.view;
    const float* __restrict__ Pm = vp.proj;

    float o_m2d[3] = { 0, 0, 0 }, o_col[3] = { 0, 0, 0 }, o_m3d[3] = { 0, 0, 0 }, o_scale[3] = { 0, 0, 0 };
    float o_conic[4] = { 0, 0, 0, 0 }, o_rot[4] = { 0, 0, 0, 0 };
    float o_cov[6] = { 0, 0, 0, 0, 0, 0 };
    float o_op = 0.f;

    {
        const float gmx = g0.x, gmy = g0.y;                 // dL/dmean2D
        const float gca = g0.z, gcb = g0.w, gcc = g1.x;     // dL/dconic (x, y, w)
        o_op = g1.y;
        o_col[0] = g1.z; o_col[1] = g1.w; o_col[2] = g2.x;
        o_m2d[0] = gmx; o_m2d[1] = gmy;
        o_conic[0] = gca; o_conic[1] = gcb; o_conic[3] = gcc;

        const float mx = means3D[3 * i], my = means3D[3 * i + 1], mz = means3D[3 * i + 2];

        // ---- recompute cov3D (forward.cu:118-152) ----
        float c3[6];
        float sx = 0, sy = 0, sz = 0, qr = 0, qx = 0, qy = 0, qz = 0;
        float raw_s[3] = { 1.f, 1.f, 1.f }, raw_inv = 1.f;      // raw mode: activated scales, 1/max(|q|, eps)
        M3 Rm = {}, Mm = {};
        if (cov3D_precomp != nullptr) {
#pragma unroll
            for (int k = 0; k < 6; k++) c3[k] = cov3D_precomp[6 * i + k];
        } else {
            sx = scales[3 * i]; sy = scales[3 * i + 1]; sz = scales[3 * i + 2];
            const float4 q = reinterpret_cast<const float4*>(rotations)[idx];
            qr = q.x; qx = q.y; qy = q.z; qz = q.w;
            if (RAW) {
                sx = act_scale(sx); sy = act_scale(sy); sz = act_scale(sz);
                raw_s[0] = sx; raw_s[1] = sy; raw_s[2] = sz;
                raw_inv = act_quat_inv_norm(qr, qx, qy, qz);
                qr *= raw_inv; qx *= raw_inv; qy *= raw_inv; qz *= raw_inv;
            }
            sx *= vp.scale_modifier; sy *= vp.scale_modifier; sz *= vp.scale_modifier;
            M3 S = { { { sx, 0, 0 }, { 0, sy, 0 }, { 0, 0, sz } } };
            Rm = quat_rotation(qr, qx, qy, qz);
            Mm = m3_mul(S, Rm);
            M3 Sig = m3_mul(m3_t(Mm), Mm);
            c3[0] = Sig.c[0][0]; c3[1] = Sig.c[0][1]; c3[2] = Sig.c[0][2];
            c3[3] = Sig.c[1][1]; c3[4] = Sig.c[1][2]; c3[5] = Sig.c[2][2];
        }

        // ---- K8: conic gradient -> cov3D gradient and mean gradient (backward.cu:159-273) ----
        const float vx = V[0] * mx + V[4] * my + V[8] * mz + V[12];
        const float vy = V[1] * mx + V[5] * my + V[9] * mz + V[13];
        const float vz = V[2] * mx + V[6] * my + V[10] * mz + V[14];
        const float limx = 1.3f * vp.tan_fovx, limy = 1.3f * vp.tan_fovy;
        const float txtz = vx / vz, tytz = vy / vz;
        const float tx = fminf(limx, fmaxf(-limx, txtz)) * vz;
        const float ty = fminf(limy, fmaxf(-limy, tytz)) * vz;
        const float x_grad_mul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
        const float y_grad_mul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
        const float h_x = vp.focal_x, h_y = vp.focal_y;
        M3 J = { { { h_x / vz, 0.0f, -(h_x * tx) / (vz * vz) },
                   { 0.0f, h_y / vz, -(h_y * ty) / (vz * vz) },
                   { 0, 0, 0 } } };
        M3 Wm = { { { V[0], V[4], V[8] }, { V[1], V[5], V[9] }, { V[2], V[6], V[10] } } };
        M3 Vrk = { { { c3[0], c3[1], c3[2] }, { c3[1], c3[3], c3[4] }, { c3[2], c3[4], c3[5] } } };
        M3 T = m3_mul(Wm, J);
        M3 cov2D = m3_mul(m3_mul(m3_t(T), m3_t(Vrk)), T);
        const float a = cov2D.c[0][0] + 0.3f, b = cov2D.c[0][1], c = cov2D.c[1][1] + 0.3f;
        const float denom = a * c - b * b;
        float dL_da = 0, dL_db = 0, dL_dc = 0;
        const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
        AACoef aa = { 0.f, 1.f, 1.f };
        float aa_drho = 0.f;
        if constexpr (AA) {
            aa = aa_coef(cov2D.c[0][0], b, cov2D.c[1][1], denom);
            const float rec_op = RAW ? act_opacity(vp.opacity_raw[i]) * aa.coef : rec_opacity;
            aa_drho = aa.rho > AA_RHO_FLOOR ? o_op * rec_op / (2.f * aa.rho) : 0.f;      // o_op is still dL/d(record opacity)
            o_op *= aa.coef;
        }
        if (denom2inv != 0) {
            dL_da = denom2inv * (-c * c * gca + 2 * b * c * gcb + (denom - a * c) * gcc);
            dL_dc = denom2inv * (-a * a * gcc + 2 * a * b * gcb + (denom - a * c) * gca);
            dL_db = denom2inv * 2 * (b * c * gca - (denom + 2 * b * b) * gcb + a * b * gcc);
            if constexpr (AA) {
                // rho = det0 / det, det0 = a0 c0 - b b, det = (a0 + h)(c0 + h) - b b; b is the one scalar dL_db refers to
                const float k = aa_drho / (denom * denom);
                dL_da += k * (cov2D.c[1][1] * denom - aa.det0 * c);
                dL_dc += k * (cov2D.c[0][0] * denom - aa.det0 * a);
                dL_db += k * (-2.f * b * (denom - aa.det0));
            }
            o_cov[0] = (T.c[0][0] * T.c[0][0] * dL_da + T.c[0][0] * T.c[1][0] * dL_db + T.c[1][0] * T.c[1][0] * dL_dc);
            o_cov[3] = (T.c[0][1] * T.c[0][1] * dL_da + T.c[0][1] * T.c[1][1] * dL_db + T.c[1][1] * T.c[1][1] * dL_dc);
            o_cov[5] = (T.c[0][2] * T.c[0][2] * dL_da + T.c[0][2] * T.c[1][2] * dL_db + T.c[1][2] * T.c[1][2] * dL_dc);
            o_cov[1] = 2 * T.c[0][0] * T.c[0][1] * dL_da + (T.c[0][0] * T.c[1][1] + T.c[0][1] * T.c[1][0]) * dL_db + 2 * T.c[1][0] * T.c[1][1] * dL_dc;
            o_cov[2] = 2 * T.c[0][0] * T.c[0][2] * dL_da + (T.c[0][0] * T.c[1][2] + T.c[0][2] * T.c[1][0]) * dL_db + 2 * T.c[1][0] * T.c[1][2] * dL_dc;
            o_cov[4] = 2 * T.c[0][2] * T.c[0][1] * dL_da + (T.c[0][1] * T.c[1][2] + T.c[0][2] * T.c[1][1]) * dL_db + 2 * T.c[1][1] * T.c[1][2] * dL_dc;
        }
        // dL/dT (upper 2x3), dL/dJ, dL/dt
        float tv0[3], tv1[3];   // T[0][k]*Vrk[j][k] sums
#pragma unroll
        for (int j = 0; j < 3; j++) {
            tv0[j] = T.c[0][0] * Vrk.c[j][0] + T.c[0][1] * Vrk.c[j][1] + T.c[0][2] * Vrk.c[j][2];
            tv1[j] = T.c[1][0] * Vrk.c[j][0] + T.c[1][1] * Vrk.c[j][1] + T.c[1][2] * Vrk.c[j][2];
        }
        const float dL_dT00 = 2 * tv0[0] * dL_da + tv1[0] * dL_db;
        const float dL_dT01 = 2 * tv0[1] * dL_da + tv1[1] * dL_db;
        const float dL_dT02 = 2 * tv0[2] * dL_da + tv1[2] * dL_db;
        const float dL_dT10 = 2 * tv1[0] * dL_dc + tv0[0] * dL_db;
        const float dL_dT11 = 2 * tv1[1] * dL_dc + tv0[1] * dL_db;
        const float dL_dT12 = 2 * tv1[2] * dL_dc + tv0[2] * dL_db;
        const float dL_dJ00 = Wm.c[0][0] * dL_dT00 + Wm.c[0][1] * dL_dT01 + Wm.c[0][2] * dL_dT02;
        const float dL_dJ02 = Wm.c[2][0] * dL_dT00 + Wm.c[2][1] * dL_dT01 + Wm.c[2][2] * dL_dT02;
        const float dL_dJ11 = Wm.c[1][0] * dL_dT10 + Wm.c[1][1] * dL_dT11 + Wm.c[1][2] * dL_dT12;
        const float dL_dJ12 = Wm.c[2][0] * dL_dT10 + Wm.c[2][1] * dL_dT11 + Wm.c[2][2] * dL_dT12;
        const float tz = 1.f / vz, tz2 = tz * tz, tz3 = tz2 * tz;
        const float dL_dtx = x_grad_mul * -h_x * tz2 * dL_dJ02;
        const float dL_dty = y_grad_mul * -h_y * tz2 * dL_dJ12;
        const float dL_dtz = -h_x * tz2 * dL_dJ00 - h_y * tz2 * dL_dJ11 + (2 * h_x * tx) * tz3 * dL_dJ02 + (2 * h_y * ty) * tz3 * dL_dJ12;
        // transformVec4x3Transpose (auxiliary.h:89-97); assigned, not accumulated (backward.cu:273)
        o_m3d[0] = V[0] * dL_dtx + V[1] * dL_dty + V[2] * dL_dtz;
        o_m3d[1] = V[4] * dL_dtx + V[5] * dL_dty + V[6] * dL_dtz;
        o_m3d[2] = V[8] * dL_dtx + V[9] * dL_dty + V[10] * dL_dtz;

        // ---- K9: screen-space mean gradient through the projection (backward.cu:370-387) ----
        const float hw = Pm[3] * mx + Pm[7] * my + Pm[11] * mz + Pm[15];
        const float m_w = 1.0f / (hw + 0.0000001f);
        const float mul1 = (Pm[0] * mx + Pm[4] * my + Pm[8] * mz + Pm[12]) * m_w * m_w;
        const float mul2 = (Pm[1] * mx + Pm[5] * my + Pm[9] * mz + Pm[13]) * m_w * m_w;
        o_m3d[0] += (Pm[0] * m_w - Pm[3] * mul1) * gmx + (Pm[1] * m_w - Pm[3] * mul2) * gmy;
        o_m3d[1] += (Pm[4] * m_w - Pm[7] * mul1) * gmx + (Pm[5] * m_w - Pm[7] * mul2) * gmy;
        o_m3d[2] += (Pm[8] * m_w - Pm[11] * mul1) * gmx + (Pm[9] * m_w - Pm[11] * mul2) * gmy;

        // ---- view-direction gradient of the SH colour -> mean (backward.cu:128-138) ----
        if (have_sh) {
            const V3 v = { mx - vp.campos[0], my - vp.campos[1], mz - vp.campos[2] }, dv = dL_ddir;
            // dnormvdv (auxiliary.h:107-117)
            const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
            const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
            o_m3d[0] += ((+sum2 - v.x * v.x) * dv.x - v.y * v.x * dv.y - v.z * v.x * dv.z) * invsum32;
            o_m3d[1] += (-v.x * v.y * dv.x + (sum2 - v.y * v.y) * dv.y - v.z * v.y * dv.z) * invsum32;
            o_m3d[2] += (-v.x * v.z * dv.x - v.y * v.z * dv.y + (sum2 - v.z * v.z) * dv.z) * invsum32;
        }
        if constexpr (DEPTH) {
            const float gz = g2.y;
            o_m3d[0] += V[2] * gz; o_m3d[1] += V[6] * gz; o_m3d[2] += V[10] * gz;
        }

        // ---- cov3D -> scale / rotation (backward.cu:278-341) ----
        if (scales != nullptr) {
            M3 dSig = { { { o_cov[0], 0.5f * o_cov[1], 0.5f * o_cov[2] },
                          { 0.5f * o_cov[1], o_cov[3], 0.5f * o_cov[4] },
                          { 0.5f * o_cov[2], 0.5f * o_cov[4], o_cov[5] } } };
            M3 M2 = Mm;
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int k = 0; k < 3; k++) M2.c[j][k] = 2.0f * Mm.c[j][k];
            M3 dL_dM = m3_mul(M2, dSig);
            M3 Rt = m3_t(Rm);
            M3 dMt = m3_t(dL_dM);
            o_scale[0] = Rt.c[0][0] * dMt.c[0][0] + Rt.c[0][1] * dMt.c[0][1] + Rt.c[0][2] * dMt.c[0][2];
            o_scale[1] = Rt.c[1][0] * dMt.c[1][0] + Rt.c[1][1] * dMt.c[1][1] + Rt.c[1][2] * dMt.c[1][2];
            o_scale[2] = Rt.c[2][0] * dMt.c[2][0] + Rt.c[2][1] * dMt.c[2][1] + Rt.c[2][2] * dMt.c[2][2];
#pragma unroll
            for (int k = 0; k < 3; k++) { dMt.c[0][k] *= sx; dMt.c[1][k] *= sy; dMt.c[2][k] *= sz; }
#define Q(a_, b_) dMt.c[a_][b_]
            o_rot[0] = 2 * qz * (Q(0, 1) - Q(1, 0)) + 2 * qy * (Q(2, 0) - Q(0, 2)) + 2 * qx * (Q(1, 2) - Q(2, 1));
            o_rot[1] = 2 * qy * (Q(1, 0) + Q(0, 1)) + 2 * qz * (Q(2, 0) + Q(0, 2)) + 2 * qr * (Q(1, 2) - Q(2, 1)) - 4 * qx * (Q(2, 2) + Q(1, 1));
            o_rot[2] = 2 * qx * (Q(1, 0) + Q(0, 1)) + 2 * qr * (Q(2, 0) - Q(0, 2)) + 2 * qz * (Q(1, 2) + Q(2, 1)) - 4 * qy * (Q(2, 2) + Q(0, 0));
            o_rot[3] = 2 * qr * (Q(0, 1) - Q(1, 0)) + 2 * qx * (Q(2, 0) + Q(0, 2)) + 2 * qy * (Q(1, 2) + Q(2, 1)) - 4 * qz * (Q(1, 1) + Q(0, 0));
#undef Q
            if (RAW) {
                // through exp: d/ds_raw = d/ds * exp(s_raw); through q = r/|r|: (g - q (q.g)) / |r|
                o_scale[0] *= raw_s[0]; o_scale[1] *= raw_s[1]; o_scale[2] *= raw_s[2];
                const float qg = qr * o_rot[0] + qx * o_rot[1] + qy * o_rot[2] + qz * o_rot[3];
                o_rot[0] = (o_rot[0] - qr * qg) * raw_inv; o_rot[1] = (o_rot[1] - qx * qg) * raw_inv;
                o_rot[2] = (o_rot[2] - qy * qg) * raw_inv; o_rot[3] = (o_rot[3] - qz * qg) * raw_inv;
            }
        }
        if (RAW) {
            const float o = act_opacity(vp.opacity_raw[i]);
            o_op *= o * (1.0f - o);
        }
    }

    // ---- interleaved accumulation (lr_views_accumulate): the five small rows of a Gaussian -- mean2D (2 of 3 floats),
    // opacity, mean3D, scale, rotation: 13 floats scattered over five arrays, each a 12-16 byte read-modify-write that
    // moves a 32-byte sector both ways -- live in ONE 64-byte row of acc16 [P][16] during the step: one full line in, one
    // out.  k_uninterleave_add hands them to the caller's tensors once per step.
    if (acc16 != nullptr) {
        float4* row = reinterpret_cast<float4*>(acc16 + 16 * i);
        float4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
        r0.x += o_m2d[0]; r0.y += o_m2d[1]; r0.z += o_op; r0.w += o_m3d[0];
        r1.x += o_m3d[1]; r1.y += o_m3d[2]; r1.z += o_scale[0]; r1.w += o_scale[1];
        r2.x += o_scale[2]; r2.y += o_rot[0]; r2.z += o_rot[1]; r2.w += o_rot[2];
        r3.x += o_rot[3];
        if constexpr (STATS) r3.y += stat_norm;
        row[0] = r0; row[1] = r1; row[2] = r2; row[3] = r3;
        return;
    }
    if constexpr (STATS) stat_accum[i] += stat_norm;
    // ---- store (or accumulate) the rows of this visible Gaussian ----
#define LR_OUT(bit, ptr, val) do { float* p__ = (ptr); *p__ = ((accum_mask >> (bit)) & 1u) ? (*p__ + (val)) : (val); } while (0)
    LR_OUT(ACC_MEAN2D, dL_dmean2D + 3 * i, o_m2d[0]); LR_OUT(ACC_MEAN2D, dL_dmean2D + 3 * i + 1, o_m2d[1]);
    if (!((accum_mask >> ACC_MEAN2D) & 1u)) dL_dmean2D[3 * i + 2] = 0.f;
    if (dL_dconic != nullptr) {
        LR_OUT(ACC_CONIC, dL_dconic + 4 * i, o_conic[0]); LR_OUT(ACC_CONIC, dL_dconic + 4 * i + 1, o_conic[1]);
        LR_OUT(ACC_CONIC, dL_dconic + 4 * i + 3, o_conic[3]);
    }
    LR_OUT(ACC_OPACITY, dL_dopacity + i, o_op);
#pragma unroll
    for (int k = 0; k < 3; k++) if (dL_dcolor != nullptr) LR_OUT(ACC_COLOR, dL_dcolor + 3 * i + k, o_col[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) LR_OUT(ACC_MEAN3D, dL_dmean3D + 3 * i + k, o_m3d[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) if (dL_dcov3D != nullptr) LR_OUT(ACC_COV3D, dL_dcov3D + 6 * i + k, o_cov[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) if (dL_dscale != nullptr) LR_OUT(ACC_SCALE, dL_dscale + 3 * i + k, o_scale[k]);
    if (dL_drot != nullptr) {
        float4* pr = reinterpret_cast<float4*>(dL_drot) + idx;
        float4 v = make_float4(o_rot[0], o_rot[1], o_rot[2], o_rot[3]);
        if ((accum_mask >> ACC_ROT) & 1u) { const float4 o = *pr; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
        *pr = v;
    }
#undef LR_OUT
}

// Persistent single-wave workgroups walk the index-ordered list of emitting Gaussians that the forward's compaction
// left in the geometry buffer (vis_list, hdr->num_compact entries), 64 Gaussians per round, rounds dealt round-robin.
// Only Gaussians that own at least one tile instance do any work or touch memory (camera paths see ~10-20 % of a
// scene; a thread-per-Gaussian launch would run the heavy body in every wave for a handful of live lanes), index
// order -- and with it the locality of the row reads/writes -- is preserved, and no global atomics are needed.
// A round is a chain of dependent memory operations (list -> slots -> rows -> LDS -> SH rows), i.e. latency bound:
// what matters is many independent rounds in flight, hence single-wave groups and a register budget of 128.
constexpr int GB_THREADS = 64;
#ifndef LR_GB_WAVES
#define LR_GB_WAVES 3
#endif
constexpr int GB_MAX_GROUPS = 256 * 4 * LR_GB_WAVES;      // CUs x SIMDs x resident waves

__device__ __forceinline__ void add4(float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

#define LR_GB_PARAMS ViewParams vp, const float* __restrict__ means3D, const float* __restrict__ scales,                          \
            const float* __restrict__ rotations, const float* __restrict__ shs,                                                 \
            const float* __restrict__ cov3D_precomp, const uint32_t* __restrict__ vis_list,                                     \
            const uint8_t* __restrict__ clamped, const uint32_t* __restrict__ offsets,                                          \
            const char* __restrict__ bin_base, const GeomHeader* __restrict__ hdr,                                              \
            float* __restrict__ dL_dmean2D, float* __restrict__ dL_dconic, float* __restrict__ dL_dopacity,                     \
            float* __restrict__ dL_dcolor, float* __restrict__ dL_dmean3D, float* __restrict__ dL_dcov3D,                       \
            float* __restrict__ dL_dsh, float* __restrict__ dL_dscale, float* __restrict__ dL_drot,                             \
            uint32_t accum_mask, float* __restrict__ acc16

// AA: the anti-aliased instantiations (gauss_backward_one); <RAW, false> is the kernel as it was
template <bool RAW, bool AA>
__global__ void __launch_bounds__(GB_THREADS) __attribute__((amdgpu_waves_per_eu(LR_GB_WAVES, 8)))
k_gauss_bwd(LR_GB_PARAMS)
{
    constexpr bool DEPTH = false, ABSG = false, STATS = false;
    constexpr float* dL_dmean2D_abs = nullptr;
    constexpr float* stat_accum = nullptr;
#include "gauss_bwd_body.h"
}
// depth mode (lr_view_backward with dL_depths and depth_image): its own entry point, so that k_gauss_bwd keeps its instruction stream
template <bool RAW, bool AA>
__global__ void __launch_bounds__(GB_THREADS) __attribute__((amdgpu_waves_per_eu(LR_GB_WAVES, 8)))
k_gauss_bwd_depth(LR_GB_PARAMS)
{
    constexpr bool DEPTH = true, ABSG = false, STATS = false;
    constexpr float* dL_dmean2D_abs = nullptr;
    constexpr float* stat_accum = nullptr;
#include "gauss_bwd_body.h"
}
// absgrad mode (lr_view_backward with dL_dmean2D_abs), with or without the depth term: own entry points again
template <bool RAW, bool AA, bool DEPTH>
__global__ void __launch_bounds__(GB_THREADS) __attribute__((amdgpu_waves_per_eu(LR_GB_WAVES, 8)))
k_gauss_bwd_abs(LR_GB_PARAMS, float* __restrict__ dL_dmean2D_abs)
{
    constexpr bool ABSG = true, STATS = false;
    constexpr float* stat_accum = nullptr;
#include "gauss_bwd_body.h"
}
// statistics mode (lr_views_accumulate with the stat_* members; activated parameters only, as that step's views are): the norm of
// the view's own screen-space gradient -- ABSG: of the slots' two absgrad sums, which are then not written anywhere -- joins the
// accumulation (gauss_backward_one<STATS>).  Own entry points once more: the kernels above keep their instruction streams.
template <bool AA, bool DEPTH, bool ABSG>
__global__ void __launch_bounds__(GB_THREADS) __attribute__((amdgpu_waves_per_eu(LR_GB_WAVES, 8)))
k_gauss_bwd_stats(LR_GB_PARAMS, float* __restrict__ stat_accum)
{
    constexpr bool RAW = false, STATS = true;
    constexpr float* dL_dmean2D_abs = nullptr;
#include "gauss_bwd_body.h"
}
#undef LR_GB_PARAMS

struct ZeroSegs { float4* p[9]; unsigned long long n4[9]; unsigned long long off[10]; int count; };

// One launch zero-fills up to nine output tensors (16-byte stores, grid-stride over the concatenation).
__global__ void __launch_bounds__(256)
k_zero_segments(ZeroSegs z)
{
    const unsigned long long total = z.off[z.count];
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (unsigned long long)gridDim.x * blockDim.x) {
        int sgi = 0;
#pragma unroll
        for (int k = 1; k < 9; k++) if (k < z.count && t >= z.off[k]) sgi = k;
        z.p[sgi][t - z.off[sgi]] = zero;
    }
}

__global__ void k_zero_tail(float* p, unsigned long long from, unsigned long long to)
{
    const unsigned long long t = from + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < to) p[t] = 0.f;
}

}  // namespace

void launch_zero_outputs(float* const* ptrs, const unsigned long long* nfloats, int count, hipStream_t s)
{
    ZeroSegs z;
    z.count = 0;
    z.off[0] = 0;
    for (int k = 0; k < count && z.count < 9; k++) {
        if (ptrs[k] == nullptr || nfloats[k] == 0) continue;
        const unsigned long long n4 = nfloats[k] / 4;          // all torch allocations are >= 16-byte aligned
        if (nfloats[k] % 4) hipLaunchKernelGGL(k_zero_tail, dim3(1), dim3(64), 0, s, ptrs[k], n4 * 4, nfloats[k]);
        if (n4 == 0) continue;
        z.p[z.count] = reinterpret_cast<float4*>(ptrs[k]);
        z.n4[z.count] = n4;
        z.off[z.count + 1] = z.off[z.count] + n4;
        z.count++;
    }
    if (z.count == 0) return;
    for (int k = z.count; k < 9; k++) { z.p[k] = nullptr; z.n4[k] = 0; z.off[k + 1] = z.off[z.count]; }
    const unsigned long long total = z.off[z.count];
    unsigned long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_zero_segments, dim3((unsigned)blocks), dim3(256), 0, s, z);
}

void launch_gauss_bwd(const ViewParams& vp, const lr_view& v, const GeomView& g, const BinView& b, const GradOut& out, bool depth,
                      bool antialiasing, hipStream_t s)
{
    if (vp.P <= 0) return;
    const dim3 grid(std::min((vp.P + GB_THREADS - 1) / GB_THREADS, GB_MAX_GROUPS)), block(GB_THREADS);
    float* const* r = out.row;
#define LR_GB_ARGS 0, s, vp, v.means3D, v.scales, v.rotations, v.shs, v.cov3D_precomp, g.vis_list, g.clamped, g.offsets, b.base,    \
                   g.header, r[ACC_MEAN2D], r[ACC_CONIC], r[ACC_OPACITY], r[ACC_COLOR], r[ACC_MEAN3D], r[ACC_COV3D], r[ACC_SH],     \
                   r[ACC_SCALE], r[ACC_ROT], out.accumulate_mask, out.acc16
    if (out.stat_accum != nullptr)
        dispatch_flags<3>(flag_bits(antialiasing, depth, out.stat_abs), [&](auto aa, auto dp, auto absg) {
            hipLaunchKernelGGL((k_gauss_bwd_stats<aa.value, dp.value, absg.value>), grid, block, LR_GB_ARGS, out.stat_accum); });
    else if (out.mean2D_abs != nullptr)
        dispatch_flags<3>(flag_bits(vp.raw != 0, antialiasing, depth), [&](auto raw, auto aa, auto dp) {
            hipLaunchKernelGGL((k_gauss_bwd_abs<raw.value, aa.value, dp.value>), grid, block, LR_GB_ARGS, out.mean2D_abs); });
    else
        dispatch_flags<3>(flag_bits(vp.raw != 0, antialiasing, depth), [&](auto raw, auto aa, auto dp) {
            if constexpr (dp.value) hipLaunchKernelGGL((k_gauss_bwd_depth<raw.value, aa.value>), grid, block, LR_GB_ARGS);
            else hipLaunchKernelGGL((k_gauss_bwd<raw.value, aa.value>), grid, block, LR_GB_ARGS); });
#undef LR_GB_ARGS
}

namespace {
// acc16 [P][16] -> the caller's accumulators (lr_views_accumulate, once per step): rows that no view touched are all
// zero and are skipped (nothing read or written on the caller's side).  STATS: float 13 of the row, the step's sum of per-view
// gradient norms (gauss_backward_one<STATS>), goes to stat_accum [P] with them.
template <bool STATS>
__global__ void __launch_bounds__(256)
k_uninterleave_add(int P, const float* __restrict__ acc16, float* __restrict__ mean2D, float* __restrict__ opacity,
                   float* __restrict__ mean3D, float* __restrict__ scale, float* __restrict__ rot, float* __restrict__ stat_accum)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float4* row = reinterpret_cast<const float4*>(acc16 + 16 * (size_t)i);
    const float4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
    const bool any = r0.x != 0.f || r0.y != 0.f || r0.z != 0.f || r0.w != 0.f || r1.x != 0.f || r1.y != 0.f || r1.z != 0.f ||
                     r1.w != 0.f || r2.x != 0.f || r2.y != 0.f || r2.z != 0.f || r2.w != 0.f || r3.x != 0.f ||
                     (STATS && r3.y != 0.f);
    if (!any) return;
    const size_t k = (size_t)i;
    if constexpr (STATS) stat_accum[k] += r3.y;
    mean2D[3 * k] += r0.x; mean2D[3 * k + 1] += r0.y;
    opacity[k] += r0.z;
    mean3D[3 * k] += r0.w; mean3D[3 * k + 1] += r1.x; mean3D[3 * k + 2] += r1.y;
    if (scale != nullptr) { scale[3 * k] += r1.z; scale[3 * k + 1] += r1.w; scale[3 * k + 2] += r2.x; }
    if (rot != nullptr) {
        float4* pr = reinterpret_cast<float4*>(rot) + i;
        float4 v = *pr;
        v.x += r2.y; v.y += r2.z; v.z += r2.w; v.w += r3.x;
        *pr = v;
    }
}
}  // namespace

void launch_uninterleave_add(int P, const float* acc16, float* mean2D, float* opacity, float* mean3D, float* scale, float* rot,
                             hipStream_t s, float* stat_accum)
{
    if (P <= 0) return;
    if (stat_accum != nullptr)
        hipLaunchKernelGGL(k_uninterleave_add<true>, dim3((P + 255) / 256), dim3(256), 0, s, P, acc16, mean2D, opacity, mean3D, scale,
                           rot, stat_accum);
    else
        hipLaunchKernelGGL(k_uninterleave_add<false>, dim3((P + 255) / 256), dim3(256), 0, s, P, acc16, mean2D, opacity, mean3D, scale,
                           rot, stat_accum);
}

}  // namespace lr
