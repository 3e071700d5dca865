"""NumPy restatement of the three MCMC densification operations (include/lucid_raster.h), written for
the tests straight from the formulas: nothing here comes from the product or from oracle/.

    dtype = np.float64 : the reference.  Inputs are the float32 raw tensors promoted to float64.
    dtype = np.float32 : the same operations in the same order in float32 -- with the double sum of the relocation's
                         denominator kept in float64, as the kernel keeps it -- for calibration: its distance from the
                         float64 result is what float32 arithmetic costs on a given input, and the tests allow the device
                         four times that.
"""
import math

import numpy as np

N_MAX = 51


def _binom_table(n=N_MAX):
    b = np.zeros((n, n), dtype=np.float64)
    for a in range(n):
        for k in range(a + 1):
            b[a, k] = float(math.comb(a, k))
    return b


BINOM = _binom_table()
WEIGHT = np.array([(-1.0) ** k / math.sqrt(k + 1) for k in range(N_MAX)], dtype=np.float64)


def sigmoid(x):
    one = x.dtype.type(1)
    return one / (one + np.exp(-x))


def new_opacity(o, N):
    """o' = 1 - (1 - o)^(1/N) as -expm1(log1p(-o) / N); o, N arrays of one dtype."""
    return -np.expm1(np.log1p(-o) / N)


def denominator(o_new, N):
    """sum_{m=1..N} sum_{k=0..m-1} C(m-1,k) (-1)^k / sqrt(k+1) o'^(k+1), in float64, powers by recurrence; o_new scalar."""
    od = np.float64(o_new)
    den = np.float64(0.0)
    for m in range(1, int(N) + 1):
        pw = od
        for k in range(m):
            den += BINOM[m - 1, k] * WEIGHT[k] * pw
            pw *= od
    return den


def split(o, N):
    """(o', s'/s) of one Gaussian of opacity o split into N, float64 scalars, no clamps: the published rule itself."""
    o = np.float64(o)
    o_new = new_opacity(o, np.float64(N))
    return o_new, o / denominator(o_new, N)


def relocate(params, moments, dst, src, min_opacity=0.005, n_max=N_MAX, dtype=np.float64):
    """params: {xyz, f_dc, f_rest, opacity, scaling, rotation} float32 arrays (any row shapes); moments: {name: array} of any
    number of further row tensors (zeroed at touched rows) or None.  Returns (params', moments') as `dtype` arrays for opacity
    and scaling and untouched copies for the rest."""
    dst, src = np.asarray(dst, dtype=np.int64), np.asarray(src, dtype=np.int64)
    out = {k: v.copy() for k, v in params.items()}
    out["opacity"] = params["opacity"].astype(dtype)
    out["scaling"] = params["scaling"].astype(dtype)
    T = dtype
    count = np.bincount(src, minlength=params["xyz"].shape[0])
    for i in np.unique(src):
        N = min(int(count[i]) + 1, n_max)
        o = min(sigmoid(params["opacity"][i].astype(T))[0], T(1.0) - T(2.0 ** -24))
        s = np.exp(params["scaling"][i].astype(T))
        o_new = new_opacity(o, T(N))
        ratio = np.float64(o) / denominator(o_new, N)
        oc = min(max(o_new, T(min_opacity)), T(1.0) - T(1.1920929e-7))
        raw_o = np.log(oc / (T(1.0) - oc))
        raw_s = np.log((s.astype(np.float64) * ratio).astype(T))
        rows = np.concatenate(([i], dst[src == i]))
        out["opacity"][rows, 0] = raw_o
        out["scaling"][rows] = raw_s
        for k in ("xyz", "f_dc", "f_rest", "rotation"):
            out[k][dst[src == i]] = params[k][i]
    mom = None
    if moments is not None:
        mom = {k: v.copy() for k, v in moments.items()}
        touched = np.concatenate((np.unique(src), dst))
        for v in mom.values():
            v[touched] = 0
    return out, mom


def gate(o):
    """g(o) = 1 / (1 + exp(-100 ((1 - o) - 0.995))): ~1 for nearly transparent Gaussians, 0 for the rest."""
    T = o.dtype.type
    with np.errstate(over="ignore"):
        return T(1) / (T(1) + np.exp(T(-100) * ((T(1) - o) - T(0.995))))


def rotation(q):
    """[P,3,3] rotation of the normalised (r,x,y,z) quaternions q / max(|q|, 1e-12)."""
    T = q.dtype.type
    n = np.maximum(np.sqrt((q * q).sum(axis=1, keepdims=True)), T(1e-12))
    r, x, y, z = ((T(1) / n) * q).T
    one, two = T(1), T(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y),
                  two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x),
                  two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)], axis=1)
    return R.reshape(-1, 3, 3)


def noise_delta(raw_scale, raw_rotation, raw_opacity, noise, scaler, dtype=np.float64):
    """Sigma xi g(o) scaler per row, Sigma = R diag(s^2) R^T evaluated as R (s^2 * (R^T xi))."""
    T = dtype
    s = np.exp(raw_scale.astype(T))
    R = rotation(raw_rotation.astype(T))
    xi = noise.astype(T)
    o = sigmoid(raw_opacity.astype(T)).reshape(-1)
    v = np.einsum("pji,pj->pi", R, xi) * (s * s)
    f = gate(o) * T(scaler)
    return np.einsum("pij,pj->pi", R, v) * f[:, None]


def noise_step(xyz, raw_scale, raw_rotation, raw_opacity, noise, scaler, dtype=np.float64):
    return xyz.astype(dtype) + noise_delta(raw_scale, raw_rotation, raw_opacity, noise, scaler, dtype)


def reg_grad(raw_opacity, raw_scale, opacity_reg, scale_reg, dtype=np.float64):
    """Gradients of opacity_reg mean(sigmoid(raw_opacity)) + scale_reg mean(exp(raw_scale)) by the closed form."""
    T = dtype
    P = raw_opacity.shape[0]
    o = sigmoid(raw_opacity.astype(T))
    w_o, w_s = T(np.float64(opacity_reg) / P), T(np.float64(scale_reg) / (3.0 * P))
    return w_o * (o * (T(1) - o)), w_s * np.exp(raw_scale.astype(T))
