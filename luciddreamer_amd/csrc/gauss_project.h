// gauss_project.h -- the per-Gaussian forward chain, ONE text for host and device: view-space point -> clip-space point -> 3D
// covariance from scale and quaternion -> EWA 2D covariance -> conic, radius, pixel centre, tile rectangle -> SH colour
// (FORWARD::preprocess, RAST/cuda_rasterizer/forward.cu:155-256, with computeCov3D :118-152, computeCov2D :74-113 and
// computeColorFromSH :20-71).  Both preprocess kernels run it; gauss_bwd.hip and mcmc.hip take the matrix helpers and the
// quaternion's rotation from here.  Every product and sum stands in the operand order of the reference source (GLM column-major
// operator order); compiled without FMA contraction (preprocess.hip; a host build with -O2 -ffp-contract=off) each is rounded on
// its own, and tests/test_gauss_project_cpu.py holds such a host build to the CPU oracle's bits without a GPU.
// NOT in here, and outside what that test pins: the loads and the raw-mode activations (common.h act_*; the device's expf is not
// the host's) -- the chain takes activated scales and the quaternion as it uses it.  The view is a template parameter: ViewParams
// (common.h), or any plain struct with its member names (view, proj, campos, tan_fovx/y, focal_x/y, W, H, gx, gy, D, M).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "screen_cull.h"          // LR_SC_HD
#if defined(__HIPCC__)
#include <hip/hip_vector_types.h>
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LR_GP_TABLE __device__ constexpr
#else
#define LR_GP_TABLE constexpr
#endif

namespace lr {

constexpr int TILE_X = 16;          // RAST/cuda_rasterizer/config.h:16-17 (tile geometry is part of the
constexpr int TILE_Y = 16;          // observable behaviour: it decides which Gaussians reach a pixel)

LR_GP_TABLE float SH_C0 = 0.28209479177387814f;
LR_GP_TABLE float SH_C1 = 0.4886025119029199f;
LR_GP_TABLE float SH_C2[5] = { 1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                               -1.0925484305920792f, 0.5462742152960396f };
LR_GP_TABLE float SH_C3[7] = { -0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                               0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                               -0.5900435899266435f };

struct M3 { float c[3][3]; };   // column-major like glm::mat3: c[col][row]
LR_SC_HD M3 m3_mul(const M3& A, const M3& B)
{
    M3 R;
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++)
            R.c[j][i] = A.c[0][i] * B.c[j][0] + A.c[1][i] * B.c[j][1] + A.c[2][i] * B.c[j][2];
    return R;
}
LR_SC_HD M3 m3_t(const M3& A)
{
    M3 R;
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) R.c[j][i] = A.c[i][j];
    return R;
}

struct V3 { float x, y, z; };
LR_SC_HD V3 operator+(V3 a, V3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
LR_SC_HD V3 operator*(float s, V3 a) { return { s * a.x, s * a.y, s * a.z }; }
LR_SC_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
LR_SC_HD V3 sh_fma(V3 acc, float s, const V3& c, bool sub = false)
{
    // acc (+|-) s * c, each product rounded separately (where contraction is off)
    V3 r;
    if (sub) { r.x = acc.x - s * c.x; r.y = acc.y - s * c.y; r.z = acc.z - s * c.z; }
    else     { r.x = acc.x + s * c.x; r.y = acc.y + s * c.y; r.z = acc.z + s * c.z; }
    return r;
}

// ---- 3D covariance (forward.cu:118-152) ----------------------------------------------------------------------------------
// The rotation of the quaternion (r, x, y, z), used as given (no normalisation here)
LR_SC_HD M3 quat_rotation(float r, float x, float y, float z)
{
    return { { { 1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y) },
               { 2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x) },
               { 2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y) } } };
}
// Sigma = (S R)^T (S R), its upper triangle in c3, from the scales with the scale modifier applied (scale_modifier * scale,
// forward.cu:123-126)
LR_SC_HD void cov3d_scale_rot(float sx, float sy, float sz, float r, float x, float y, float z, float (&c3)[6])
{
    M3 S = { { { sx, 0, 0 }, { 0, sy, 0 }, { 0, 0, sz } } };
    M3 Mm = m3_mul(S, quat_rotation(r, x, y, z));
    M3 Sig = m3_mul(m3_t(Mm), Mm);
    c3[0] = Sig.c[0][0]; c3[1] = Sig.c[0][1]; c3[2] = Sig.c[0][2];
    c3[3] = Sig.c[1][1]; c3[4] = Sig.c[1][2]; c3[5] = Sig.c[2][2];
}

// ---- EWA 2D covariance (forward.cu:74-113) of the view-space point (vx, vy, vz): T^T Vrk^T T, its 2 x 2 part, undilated ----
template <class View>
LR_SC_HD M3 ewa_cov2d(const View& vp, float vx, float vy, float vz, const float (&c3)[6])
{
    const float* __restrict__ V = vp.view;
    const float limx = 1.3f * vp.tan_fovx, limy = 1.3f * vp.tan_fovy;
    const float txtz = vx / vz, tytz = vy / vz;
    const float tx = fminf(limx, fmaxf(-limx, txtz)) * vz;
    const float ty = fminf(limy, fmaxf(-limy, tytz)) * vz;
    M3 J = { { { vp.focal_x / vz, 0.0f, -(vp.focal_x * tx) / (vz * vz) },
               { 0.0f, vp.focal_y / vz, -(vp.focal_y * ty) / (vz * vz) },
               { 0, 0, 0 } } };
    M3 Wm = { { { V[0], V[4], V[8] }, { V[1], V[5], V[9] }, { V[2], V[6], V[10] } } };
    M3 T = m3_mul(Wm, J);
    M3 Vrk = { { { c3[0], c3[1], c3[2] }, { c3[1], c3[3], c3[4] }, { c3[2], c3[4], c3[5] } } };
    return m3_mul(m3_mul(m3_t(T), m3_t(Vrk)), T);
}

// ---- anti-aliasing (lr_set_antialiasing): opacity compensation for the 2D dilation ---------------------------------------
// The screen-space covariance {a0, b, c0} is dilated by AA_DILATION on its diagonal before it is inverted (forward.cu:219), which
// spreads a splat without dimming it.  With anti-aliasing on the record's opacity is multiplied by coef = sqrt(max(AA_RHO_FLOOR,
// det0 / det)), det0 / det the determinants before / after the dilation (the 2D Mip filter of Mip-Splatting).  ONE definition,
// every operation rounded on its own in this order whatever the contraction setting of the translation unit: tests/aa_ref.py
// restates it operation for operation.  `det` = (a0 + h) (c0 + h) - b b as the chain forms it.
constexpr float AA_DILATION = 0.3f;
constexpr float AA_RHO_FLOOR = 0.000025f;
struct AACoef { float det0, rho, coef; };
LR_SC_HD AACoef aa_coef(float a0, float b, float c0, float det)
{
#pragma clang fp contract(off)
    AACoef r;
    r.det0 = a0 * c0 - b * b;
    r.rho = r.det0 / det;
    r.coef = sqrtf(fmaxf(AA_RHO_FLOOR, r.rho));
    return r;
}

// ---- tile rectangle of a splat (RAST/cuda_rasterizer/auxiliary.h:46-56) -------------------------------------------------------
LR_SC_HD int gp_min(int a, int b) { return a < b ? a : b; }
LR_SC_HD int gp_max(int a, int b) { return a > b ? a : b; }
LR_SC_HD void tile_rect(float px, float py, int radius, int gx, int gy, int& minx, int& miny, int& maxx, int& maxy)
{
    minx = gp_min(gx, gp_max(0, (int)((px - radius) / TILE_X)));
    miny = gp_min(gy, gp_max(0, (int)((py - radius) / TILE_Y)));
    maxx = gp_min(gx, gp_max(0, (int)((px + radius + TILE_X - 1) / TILE_X)));
    maxy = gp_min(gy, gp_max(0, (int)((py + radius + TILE_Y - 1) / TILE_Y)));
}

// ---- the projection chain proper (forward.cu:196-232) ------------------------------------------------------------------------
// What it leaves of a Gaussian.  coef: anti-aliased kernels only.
struct GaussProj { float pix, piy, con_a, con_b, con_c, vz; int radius; float coef; };

// One Gaussian that passed the near plane, from its world position and 3D covariance.  false: culled (det == 0 or empty tile
// rectangle).
template <bool AA, class View>
LR_SC_HD bool project_chain(const View& vp, float px_w, float py_w, float pz_w, const float (&c3)[6], GaussProj& out)
{
    const float* __restrict__ V = vp.view;
    const float* __restrict__ Pm = vp.proj;
    // view-space point (auxiliary.h:58-66)
    const float vx = V[0] * px_w + V[4] * py_w + V[8] * pz_w + V[12];
    const float vy = V[1] * px_w + V[5] * py_w + V[9] * pz_w + V[13];
    const float vz = V[2] * px_w + V[6] * py_w + V[10] * pz_w + V[14];
    // clip-space projection (forward.cu:196-200)
    const float hx = Pm[0] * px_w + Pm[4] * py_w + Pm[8] * pz_w + Pm[12];
    const float hy = Pm[1] * px_w + Pm[5] * py_w + Pm[9] * pz_w + Pm[13];
    const float hw = Pm[3] * px_w + Pm[7] * py_w + Pm[11] * pz_w + Pm[15];
    const float p_w = 1.0f / (hw + 0.0000001f);
    const float ndcx = hx * p_w, ndcy = hy * p_w;

    const M3 cov = ewa_cov2d(vp, vx, vy, vz, c3);
    const float ca = cov.c[0][0] + 0.3f, cb = cov.c[0][1], cc = cov.c[1][1] + 0.3f;

    const float det = ca * cc - cb * cb;                   // forward.cu:219-223
    if (det == 0.0f) return false;
    const float det_inv = 1.f / det;
    out.con_a = cc * det_inv; out.con_b = -cb * det_inv; out.con_c = ca * det_inv;
    if constexpr (AA) out.coef = aa_coef(cov.c[0][0], cb, cov.c[1][1], det).coef;

    const float mid = 0.5f * (ca + cc);                    // forward.cu:229-232
    const float lambda1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
    const float lambda2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
    const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
    // ndc2Pix evaluates in double (auxiliary.h:41-44)
    out.pix = (float)(((ndcx + 1.0) * vp.W - 1.0) * 0.5);
    out.piy = (float)(((ndcy + 1.0) * vp.H - 1.0) * 0.5);
    out.radius = (int)my_radius;
    out.vz = vz;
    int minx, miny, maxx, maxy;
    tile_rect(out.pix, out.piy, out.radius, vp.gx, vp.gy, minx, miny, maxx, maxy);
    return (uint32_t)(maxx - minx) * (uint32_t)(maxy - miny) != 0u;
}

// ---- colour (forward.cu:20-71) ---------------------------------------------------------------------------------------------------
// one 16-byte load: the device's float4 (a vector_size type changes both kernels' instruction streams), its like on the host
#if defined(__HIPCC__)
typedef float4 gp_f4;
#else
struct alignas(16) gp_f4 { float x, y, z, w; };
#endif

// Load K coefficient triples of Gaussian idx.  M==16 rows are 192 B (16-byte aligned): 12 x dwordx4.
template <int K>
LR_SC_HD void load_sh(const float* __restrict__ shs, size_t idx, int M, V3 (&sh)[16])
{
    const float* base = shs + idx * (size_t)M * 3;
    constexpr int NF = 3 * K;
    float f[(NF + 3) / 4 * 4];
    if (((M * 3) & 3) == 0 && ((reinterpret_cast<uintptr_t>(shs) & 15) == 0)) {
        const gp_f4* b4 = reinterpret_cast<const gp_f4*>(base);
#pragma unroll
        for (int q = 0; q < (NF + 3) / 4; q++) {
            gp_f4 v = b4[q];
            f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < NF; q++) f[q] = base[q];
    }
#pragma unroll
    for (int k = 0; k < K; k++) { sh[k].x = f[3 * k]; sh[k].y = f[3 * k + 1]; sh[k].z = f[3 * k + 2]; }
}

// raw mode: coefficient 0 from features_dc [P,3], coefficients 1.. from features_rest [P,M-1,3]
template <int K>
LR_SC_HD void load_sh_split(const float* __restrict__ dc, const float* __restrict__ rest, size_t idx, int M, V3 (&sh)[16])
{
    sh[0].x = dc[3 * idx]; sh[0].y = dc[3 * idx + 1]; sh[0].z = dc[3 * idx + 2];
    const float* base = rest + idx * (size_t)(M - 1) * 3;
#pragma unroll
    for (int k = 1; k < K; k++) { sh[k].x = base[3 * (k - 1)]; sh[k].y = base[3 * (k - 1) + 1]; sh[k].z = base[3 * (k - 1) + 2]; }
}

template <int DEG>
LR_SC_HD V3 eval_sh(const float* __restrict__ shs, const float* __restrict__ sh_rest, size_t idx, int M, V3 dir, uint8_t& clamp_bits)
{
    V3 sh[16];
    if (sh_rest != nullptr) load_sh_split<(DEG + 1) * (DEG + 1)>(shs, sh_rest, idx, M, sh);
    else load_sh<(DEG + 1) * (DEG + 1)>(shs, idx, M, sh);
    V3 res = { SH_C0 * sh[0].x, SH_C0 * sh[0].y, SH_C0 * sh[0].z };
    if (DEG > 0) {
        float x = dir.x, y = dir.y, z = dir.z;
        res = sh_fma(res, SH_C1 * y, sh[1], true);
        res = sh_fma(res, SH_C1 * z, sh[2]);
        res = sh_fma(res, SH_C1 * x, sh[3], true);
        if (DEG > 1) {
            float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            res = sh_fma(res, SH_C2[0] * xy, sh[4]);
            res = sh_fma(res, SH_C2[1] * yz, sh[5]);
            res = sh_fma(res, SH_C2[2] * (2.0f * zz - xx - yy), sh[6]);
            res = sh_fma(res, SH_C2[3] * xz, sh[7]);
            res = sh_fma(res, SH_C2[4] * (xx - yy), sh[8]);
            if (DEG > 2) {
                res = sh_fma(res, SH_C3[0] * y * (3.0f * xx - yy), sh[9]);
                res = sh_fma(res, SH_C3[1] * xy * z, sh[10]);
                res = sh_fma(res, SH_C3[2] * y * (4.0f * zz - xx - yy), sh[11]);
                res = sh_fma(res, SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy), sh[12]);
                res = sh_fma(res, SH_C3[4] * x * (4.0f * zz - xx - yy), sh[13]);
                res = sh_fma(res, SH_C3[5] * z * (xx - yy), sh[14]);
                res = sh_fma(res, SH_C3[6] * x * (xx - 3.0f * yy), sh[15]);
            }
        }
    }
    res.x += 0.5f; res.y += 0.5f; res.z += 0.5f;
    clamp_bits = (uint8_t)((res.x < 0 ? 1 : 0) | (res.y < 0 ? 2 : 0) | (res.z < 0 ? 4 : 0));
    res.x = fmaxf(res.x, 0.0f); res.y = fmaxf(res.y, 0.0f); res.z = fmaxf(res.z, 0.0f);
    return res;
}

// Colour of the Gaussian at world position (px_w, py_w, pz_w) from its SH rows: the view direction from vp.campos, degree
// vp.D of vp.M coefficients.  sh_rest != nullptr: the split rows of raw mode (load_sh_split).
template <class View>
LR_SC_HD V3 sh_colour(const View& vp, const float* __restrict__ shs, const float* __restrict__ sh_rest, size_t idx,
                      float px_w, float py_w, float pz_w, uint8_t& clamp_bits)
{
    V3 dir = { px_w - vp.campos[0], py_w - vp.campos[1], pz_w - vp.campos[2] };
    const float len = sqrtf(dir.x * dir.x + dir.y * dir.y + dir.z * dir.z);
    dir.x = dir.x / len; dir.y = dir.y / len; dir.z = dir.z / len;
    switch (vp.D) {
        case 0: return eval_sh<0>(shs, sh_rest, idx, vp.M, dir, clamp_bits);
        case 1: return eval_sh<1>(shs, sh_rest, idx, vp.M, dir, clamp_bits);
        case 2: return eval_sh<2>(shs, sh_rest, idx, vp.M, dir, clamp_bits);
        default: return eval_sh<3>(shs, sh_rest, idx, vp.M, dir, clamp_bits);
    }
}

}  // namespace lr
