// screen_cull.h -- a conservative "this splat cannot reach the screen" test, cheap enough for phase 1 of the pooled
// preprocess kernel (preprocess.hip k_preprocess_pool).  One header for host and device: + - x and comparisons only (and |x|; no
// division, no square root, no reciprocal), so a host build with -ffp-contract=off takes the same decision bit for bit
// (tests/test_screen_cull_cpu.py holds it against the oracle's radii).
//
// screen_cull_reject() returns true ONLY when the exact chain (preprocess.hip project_gaussian, forward.cu:196-232) would
// certainly return false because its tile rectangle is empty.  Everything it cannot decide -- NaN, inf, hw' <= 0, absurd
// scales -- passes (returns false), and the exact chain runs on it as before.
//
// The exact chain, in real numbers:
//   pix = (hx / hw' + 1) W / 2 - 1/2                      hw' = hw + 1e-7 (the chain's own p_w = 1 / hw')
//   cov = [J W Sigma W^T J^T] (2 x 2),  Sigma = (S R(q))^T (S R(q)),  a = cov00 + 0.3,  c = cov11 + 0.3
//   lambda1 = mid + sqrt(max(0.1, mid^2 - det)),  mid = (a + c) / 2,  radius = ceil(3 sqrt(lambda1))
//   tile_rect: empty when  pix + radius + 15 < 16  (max x = 0)  or  pix - radius >= 16 gx  (min x = gx); the same in y.
// tile_rect is monotone in the radius (min x, min y do not grow and max x, max y do not shrink with it), so an empty
// rectangle for a LARGER radius implies an empty rectangle for the true one: an upper bound of the radius is enough.
//
// Radius bound.  det >= 0 for a positive semi-definite cov, so sqrt(mid^2 - det) <= mid, and sqrt(max(0.1, x)) <=
//   sqrt(0.1) + sqrt(max(0, x)):  lambda1 <= 2 mid + sqrt(0.1) = (cov00 + cov11 + 0.6) + sqrt(0.1); this includes the 0.1
//   floor.  ceil(x) < x + 1:  radius < 3 sqrt(lambda1) + 1.
// Covariance bound.  cov00 + cov11 = sum_i t_i^T Sigma t_i over the two rows t_i of J W
//   <= ||J W||_F^2 ||Sigma||_2 <= ||J||_F^2 ||W||_F^2 ||R(q)||_2^2 s^2,   s = |scale_modifier| max_i |scale_i| = ||S||_2.
// Jacobian bound.  J = [[fx / vz, 0, -fx tx / vz^2], [0, fy / vz, -fy ty / vz^2]] with tx / vz, ty / vz clamped to
//   +-1.3 tan_fov = lim:  ||J||_F^2 <= (fx^2 (1 + limx^2) + fy^2 (1 + limy^2)) / vz^2 = g / vz^2.
// Rotation bound.  For ANY quaternion q = (r, x, y, z) with n = |q|^2 the chain's matrix is R(q) = n Rot(q / |q|) + (1 - n) I
//   (diagonal: 1 - 2 (y^2 + z^2) = (r^2 + x^2 - y^2 - z^2) + (1 - n); the off-diagonal entries are those of n Rot), so
//   ||R(q)||_2 <= n + |1 - n|  (1 for a unit quaternion, never more than 1 + 2 n).  q = 0 gives R = I: bound 1.
// View bound.  ||W||_F^2 is summed from the nine entries of the view matrix as given (3 for a rigid view); nothing is assumed.
//
// Squared form.  "Left of the screen" with the bounds above and a margin of m pixels:
//       pix + m + 3 sqrt(L) < 0,        L = 0.6 + sqrt(0.1) + g ||W||_F^2 (s ||R||)^2 / vz^2 >= lambda1.
//   Multiply by hw' > 0 and vz > 0:   vz ((hx + hw') W/2 + (m - 1/2) hw') + 3 hw' sqrt(vz^2 L) < 0,  that is with
//       B = -vz ((hx + hw') W/2 + (m - 1/2) hw'),   A = hw'^2 (C0 vz^2 + g ||W||_F^2 (s ||R||)^2):    B > 0  and  9 A < B^2.
//   "Right of the screen":  pix - 3 sqrt(L) - 1 - m - 16 gx > 0  gives  B = vz ((hx + hw') W/2 - (16 gx + 3/2 + m) hw').
//   With c = (hx + hw') W/2, m_lo = m - 1/2 and m_hi = 16 gx + 3/2 + m the two are B = vz (-c - m_lo hw') and
//   B = vz (c - m_hi hw'); they exclude each other, and their maximum is
//       B = vz (|c - k hw'| - e hw'),   k = (m_hi - m_lo) / 2,  e = (m_hi + m_lo) / 2      (one test per axis).
//   Top and bottom alike with hy, H, gy.
// Margins.  m = 2 pixels and a relative 1e-3 on A (5e-4 on the radius).  They cover the float32 rounding of the exact
//   chain -- p_w and ndc carry 2^-23 each, pix one more rounding (absolute error ~2e-7 (|pix| + W)), the covariance
//   products ~1e-5 relative, a float det a few ulp below zero -- and the rounding of B and A themselves (a few 2^-24 of
//   their terms).  Near the screen (|pix| < 1e6) the pixel margin is the larger one; farther out the radius that could still
//   reach the screen is ~|pix| and the relative margin (5e-4 |pix|) exceeds every rounding term (~1e-6 |pix|).  hx, hy, hw'
//   and vz must be computed by the chain's own expressions (same operand order, no contraction): they are then its bits.
// NaN / inf.  Every comparison is written so that NaN makes it false and every false means "pass"; products that overflow
//   make A = inf (9 A < B^2 is false) or B = inf with A = inf.  Scales beyond 1e9 pass outright: there the chain's own
//   intermediates may overflow where this bound's do not.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LR_SC_HD __host__ __device__ __forceinline__
#else
#define LR_SC_HD inline
#endif

namespace lr {

constexpr float SC_PIX_MARGIN = 2.0f;
constexpr float SC_NINE = 9.0f * 1.001f;            // 9 A with the relative margin folded in
constexpr float SC_C0 = 0.9163f;                    // >= 0.6 + sqrt(0.1) = 0.916228
constexpr float SC_S_MAX = 1e9f;

// Per-view constants (api.hip fills them where ViewParams is filled; the view matrix lives on the device, so ||W||_F^2 is
// summed in the kernel: screen_cull_wf).
struct ScreenCull {
    float g;                // fx^2 (1 + limx^2) + fy^2 (1 + limy^2)
    float half_w, half_h;   // W / 2, H / 2
    float kx, ex;           // (m_hi - m_lo) / 2 and (m_hi + m_lo) / 2 with m_lo = m - 1/2, m_hi = 16 gx + 3/2 + m (see below)
    float ky, ey;           // ... with 16 gy
};

inline ScreenCull screen_cull_view(int W, int H, int gx, int gy, float tan_fovx, float tan_fovy, float focal_x, float focal_y)
{
    const float limx = 1.3f * tan_fovx, limy = 1.3f * tan_fovy;
    ScreenCull c;
    c.g = focal_x * focal_x * (1.0f + limx * limx) + focal_y * focal_y * (1.0f + limy * limy);
    c.half_w = 0.5f * (float)W; c.half_h = 0.5f * (float)H;
    const float m_lo = SC_PIX_MARGIN - 0.5f;
    const float m_hx = 16.0f * (float)gx + 1.5f + SC_PIX_MARGIN, m_hy = 16.0f * (float)gy + 1.5f + SC_PIX_MARGIN;
    c.kx = 0.5f * (m_hx - m_lo); c.ex = 0.5f * (m_hx + m_lo);
    c.ky = 0.5f * (m_hy - m_lo); c.ey = 0.5f * (m_hy + m_lo);
    return c;
}

// ||W||_F^2 of the view matrix's 3 x 3 part (flat index m[4 * col + row])
LR_SC_HD float screen_cull_wf(const float* V)
{
    return V[0] * V[0] + V[1] * V[1] + V[2] * V[2] + V[4] * V[4] + V[5] * V[5] + V[6] * V[6] + V[8] * V[8] + V[9] * V[9] +
           V[10] * V[10];
}

// s = |scale_modifier| max_i |scale_i|; NaN when any scale is NaN or infinite (fmaxf alone would drop a NaN)
LR_SC_HD float screen_cull_scale(float scale_modifier, float sx, float sy, float sz)
{
    const float mx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(sx), __builtin_fabsf(sy)), __builtin_fabsf(sz));
    return __builtin_fabsf(scale_modifier) * mx + (sx + sy + sz) * 0.0f;
}

LR_SC_HD float screen_cull_qn2(float r, float x, float y, float z) { return r * r + x * x + y * y + z * z; }

// true: the tile rectangle of this Gaussian is certainly empty.  kv9 = SC_NINE * c.g * ||W||_F^2 (once per wave);
// hwp = hw + 0.0000001f; s from screen_cull_scale; qn2 = |q|^2 of the quaternion the chain uses.
// (& and | on purpose: straight-line code, no short-circuit branches; |x| is exact and counts as a comparison.)
LR_SC_HD bool screen_cull_reject(const ScreenCull& c, float kv9, float hx, float hy, float hwp, float vz, float s, float qn2)
{
    const float rb = qn2 + __builtin_fabsf(1.0f - qn2);              // >= ||R(q)||_2
    const float sr = s * rb;
    const float a9 = (hwp * hwp) * ((SC_NINE * SC_C0) * (vz * vz) + kv9 * (sr * sr));      // 9 A (1 + 1e-3)
    // one test per axis: left and right (top and bottom) exclude each other
    const float ux = __builtin_fabsf((hx + hwp) * c.half_w - c.kx * hwp) - c.ex * hwp;
    const float uy = __builtin_fabsf((hy + hwp) * c.half_h - c.ky * hwp) - c.ey * hwp;
    const float bx = vz * ux, by = vz * uy;
    const bool off = ((bx > 0.0f) & (a9 < bx * bx)) | ((by > 0.0f) & (a9 < by * by));
    return off & (hwp > 0.0f) & (vz > 0.0f) & (sr <= SC_S_MAX);
}

// The test for one Gaussian, from what phase 1 of the pooled kernel holds: world position, its view-space depth vz (the
// near-plane test's own value), the scales and the quaternion as the chain uses them (activated / normalised in raw mode).
// hx, hy, hw are the chain's own expressions (project_gaussian), so with contraction off they are its bits.
LR_SC_HD bool screen_cull_point(const ScreenCull& c, float kv9, const float* Pm, float scale_modifier, float px_w, float py_w,
                                float pz_w, float vz, float sx, float sy, float sz, float qr, float qx, float qy, float qz)
{
    const float hx = Pm[0] * px_w + Pm[4] * py_w + Pm[8] * pz_w + Pm[12];
    const float hy = Pm[1] * px_w + Pm[5] * py_w + Pm[9] * pz_w + Pm[13];
    const float hw = Pm[3] * px_w + Pm[7] * py_w + Pm[11] * pz_w + Pm[15];
    return screen_cull_reject(c, kv9, hx, hy, hw + 0.0000001f, vz, screen_cull_scale(scale_modifier, sx, sy, sz),
                              screen_cull_qn2(qr, qx, qy, qz));
}

// kv9 of a view: the margin, the Jacobian constant and ||W||_F^2 in one factor
LR_SC_HD float screen_cull_kv9(const ScreenCull& c, const float* V) { return SC_NINE * c.g * screen_cull_wf(V); }

}  // namespace lr
