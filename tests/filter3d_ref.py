"""NumPy restatement of the 3D smoothing filter (include/lucid_raster.h lr_filter3d_*), written for
the tests straight from the formulas: nothing here comes from the product or from oracle/.

    dtype = np.float64 : the reference.  Inputs are the float32 tensors promoted to float64; the apply's reference uses the
                         plain closed forms (s' = sqrt(s^2 + f^2) through logs that cannot cancel), not the kernel's branches.
    dtype = np.float32 : the kernel's operations in the kernel's order in float32, for calibration: its distance from the
                         float64 result is what float32 arithmetic costs on a given input, and the tests allow the device four
                         times that.  For update() it is more: the kernel is compiled without FMA contraction and uses only
                         correctly rounded operations there, so this restatement is what the device computes.

cams is the packed [V,20] array of filter3d.pack_cameras: 16 matrix floats (row-vector convention), fx, fy, W, H.
"""
import numpy as np

NEAR, MARGIN = 0.2, 0.65
FRAGILE_REL = 1e-4


def view_space(xyz, cams, dtype=np.float64):
    """x, y, z [P,V] as ((M0j px + M1j py) + M2j pz) + M3j in `dtype`."""
    p = xyz.astype(dtype)
    M = cams[:, :16].astype(dtype).reshape(-1, 4, 4)
    px, py, pz = p[:, None, 0], p[:, None, 1], p[:, None, 2]
    return tuple(((M[None, :, 0, j] * px + M[None, :, 1, j] * py) + M[None, :, 2, j] * pz) + M[None, :, 3, j] for j in range(3))


def update(xyz, cams, variance=0.2, dtype=np.float64, return_fragile=False):
    """(filter [P] dtype, seen [P] bool[, fragile [P,V] bool]).  A pair is fragile when z is within 1e-4 relative of 0.2 or a
    projected coordinate within 1e-4 relative of its 0.65 bound: float32 may land on the other side of the test there."""
    T = dtype
    P, V = xyz.shape[0], cams.shape[0]
    if V == 0:
        out = (np.zeros(P, T), np.zeros(P, bool))
        return out + (np.zeros((P, 0), bool),) if return_fragile else out
    x, y, z = view_space(xyz, cams, T)
    c = cams.astype(T)
    fx, fy, W, H = c[None, :, 16], c[None, :, 17], c[None, :, 18], c[None, :, 19]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = np.abs(x / z * fx), np.abs(y / z * fy)
        bu, bv = T(MARGIN) * W, T(MARGIN) * H
        front = z > T(NEAR)
        sees = front & (u <= bu) & (v <= bv)
        d = np.where(sees, z / fx, T(np.inf)).min(axis=1)
    seen = sees.any(axis=1)
    sv = np.sqrt(T(variance))
    widest = sv * d[seen].max() if seen.any() else T(0)
    filt = np.where(seen, sv * np.where(seen, d, T(0)), widest).astype(T)
    if not return_fragile:
        return filt, seen
    with np.errstate(invalid="ignore"):
        near_z = np.abs(z - NEAR) <= FRAGILE_REL * NEAR
        # a projected coordinate only matters in front of the camera (behind it the pair is unseen whatever it is)
        near_u = front & (np.abs(u - bu) <= FRAGILE_REL * bu)
        near_v = front & (np.abs(v - bv) <= FRAGILE_REL * bv)
    return filt, seen, near_z | near_u | near_v


def sigmoid(x):
    one = x.dtype.type(1)
    return one / (one + np.exp(-x))


# ---- float64 reference of the apply ---------------------------------------------------------------------------------------
def apply64(raw_scale, raw_opacity, filt, activated):
    """(scale out [P,3], opacity out [P]) in float64 from the definitions: s'^2 = s^2 + f^2, o' = sigmoid(q) sqrt(prod s^2 /
    prod s'^2); stored = (log s', logit o').  Rows with f == 0 are the inputs (activated: their activations)."""
    r, q, f = raw_scale.astype(np.float64), raw_opacity.astype(np.float64).reshape(-1), filt.astype(np.float64).reshape(-1, 1)
    with np.errstate(divide="ignore", over="ignore"):
        # log s' = logaddexp(2 r, 2 log f) / 2: exact in the sense that nothing cancels and nothing overflows
        log_s = np.where(f > 0, 0.5 * np.logaddexp(2 * r, 2 * np.log(np.where(f > 0, f, 1.0))), r)
    log_c = (r - log_s).sum(axis=1)                                   # <= 0
    log_sig = -np.logaddexp(0.0, -q)
    if activated:
        return np.exp(log_s), np.exp(log_sig + log_c)
    # logit o' = log o' - log(1 - o'), 1 - o' = sigmoid(-q) + sigmoid(q) (1 - c)
    one_minus = sigmoid(-q) + sigmoid(q) * (-np.expm1(log_c))
    logit = np.where(f[:, 0] > 0, log_sig + log_c - np.log(one_minus), q)
    return log_s, logit


def backward64(raw_scale, raw_opacity, filt, g_scale, g_opacity, activated):
    """The issue's table in float64: (dL/dr [P,3], dL/dq [P])."""
    r, q, f = raw_scale.astype(np.float64), raw_opacity.astype(np.float64).reshape(-1), filt.astype(np.float64).reshape(-1, 1)
    g, go = g_scale.astype(np.float64), g_opacity.astype(np.float64).reshape(-1)
    with np.errstate(over="ignore", divide="ignore"):
        # w = t / (1 + t) = sigmoid(log t), u = sigmoid(-log t), log t = 2 (log f - r)
        log_t = np.where(f > 0, 2 * (np.log(np.where(f > 0, f, 1.0)) - r), -np.inf)
        w = np.where(f > 0, 1.0 / (1.0 + np.exp(-log_t)), 0.0)
        u = np.where(f > 0, 1.0 / (1.0 + np.exp(log_t)), 1.0)
    s_out, o_out = apply64(raw_scale, raw_opacity, filt, True)
    sig, nsig = sigmoid(q), sigmoid(-q)
    if activated:
        c = np.exp((r - np.log(s_out)).sum(axis=1))
        return g * s_out * u + (go * o_out)[:, None] * w, go * c * sig * nsig
    log_c = (r - np.log(s_out)).sum(axis=1)
    one_minus = nsig + sig * (-np.expm1(log_c))
    return g * u + (go / one_minus)[:, None] * w, go * nsig / one_minus


# ---- float32 restatement of the kernels -----------------------------------------------------------------------------------
def _terms32(r, q, f):
    """f3_terms of csrc/filter3d.hip on arrays: r [P,3], q [P], f [P] float32 with f > 0."""
    F = np.float32
    f = f[:, None]
    f2, log_f = f * f, np.log(f)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        t = f2 * np.exp(F(-2) * r)
        small = t <= F(1)
        ts = np.where(small, t, F(0))
        it = np.where(small, F(0), F(1) / np.where(small, F(1), t))
        inv_s, inv_l = F(1) / (F(1) + ts), F(1) / (F(1) + it)
        h = np.where(small, F(0.5) * np.log1p(ts), (log_f - r) + F(0.5) * np.log1p(it))
        u = np.where(small, inv_s, it * inv_l)
        w = np.where(small, ts * inv_s, inv_l)
    log_c = -((h[:, 0] + h[:, 1]) + h[:, 2])
    e = np.exp(-np.abs(q))
    inv = F(1) / (F(1) + e)
    sig = np.where(q >= 0, inv, e * inv)
    nsig = np.where(q >= 0, e * inv, inv)
    log_sig = np.minimum(q, F(0)) - np.log1p(e)
    one_minus = nsig + sig * (-np.expm1(log_c))
    return h.astype(F), u.astype(F), w.astype(F), log_c.astype(F), sig.astype(F), nsig.astype(F), log_sig.astype(F), one_minus.astype(F)


def _as32(raw_scale, raw_opacity, filt):
    F = np.float32
    return raw_scale.astype(F), raw_opacity.astype(F).reshape(-1), filt.astype(F).reshape(-1)


def apply32(raw_scale, raw_opacity, filt, activated):
    F = np.float32
    r, q, f = _as32(raw_scale, raw_opacity, filt)
    on = f > 0
    h, u, w, log_c, sig, nsig, log_sig, one_minus = _terms32(r, q, np.where(on, f, F(1)))
    with np.errstate(over="ignore"):
        if activated:
            s = np.where(on[:, None], np.exp(r + h), np.exp(r))
            o = np.where(on, sig * np.exp(log_c), F(1) / (F(1) + np.exp(-q)))
        else:
            s = np.where(on[:, None], r + h, r)
            o = np.where(on, (log_sig + log_c) - np.log(one_minus), q)
    return s.astype(F), o.astype(F)


def backward32(raw_scale, raw_opacity, filt, g_scale, g_opacity, activated):
    F = np.float32
    r, q, f = _as32(raw_scale, raw_opacity, filt)
    g, go = g_scale.astype(F), g_opacity.astype(F).reshape(-1)
    on = f > 0
    h, u, w, log_c, sig, nsig, log_sig, one_minus = _terms32(r, q, np.where(on, f, F(1)))
    gc = go[:, None]
    with np.errstate(over="ignore"):
        if activated:
            c = np.exp(log_c)
            o = sig * c
            dr = np.where(on[:, None], g * np.exp(r + h) * u + gc * o[:, None] * w, g * np.exp(r))
            s0 = F(1) / (F(1) + np.exp(-q))
            dq = np.where(on, go * c * (sig * nsig), go * (s0 * (F(1) - s0)))
        else:
            dr = np.where(on[:, None], g * u + gc * w / one_minus[:, None], g)
            dq = np.where(on, go * nsig / one_minus, go)
    return dr.astype(F), dq.astype(F)
