"""Plain numpy restatement of the dreaming kernels (csrc/dream.hip; luciddreamer_amd.reproject.fit_scale, scatter_interpolate,
compensate, dream_step), operation for operation.

Every float64 expression is written elementwise in the order the header documents (include/lucid_raster.h, lr_dream_* and
lr_scatter_interpolate), so numpy forms the same bits as the device: no BLAS, no fused multiply-add, no np.sum (pairwise).  The
sums over samples are sequential `for j` loops, vectorised over the pixels; the scale sums follow the device's tree.

    liftw(x, y, d, K, R, T)                         -> 3 float64 arrays
    scale_terms / scale_sums / fit_from_sums        -> (a)
    correspond(X, pix, corr, D, K, R, T, H, W, s)   -> su, sv, sval  float64 [M + 4]                       (b)
    scatter(su, sv, sval, H, W, where)              -> float32 [H,W]                                      (c)
    dream_lift(D, nd, K, R, T, s)                   -> float32 [3, H*W]                                   (d)
    border_corr(frame) / compensate / dream_step    -> the Python layer; `frame` is reproject_ref.project()'s dict
"""
import math

import numpy as np

from tests import reproject_ref as RR

BLOCK = 256                  # points per workgroup of the scale sums = samples per tile of the interpolation (LR_SCATTER_TILE)


def _pose_inverses(K, R, T):
    Ki = np.linalg.inv(np.asarray(K, dtype=np.float64).reshape(3, 3))
    Ri = np.linalg.inv(np.asarray(R, dtype=np.float64).reshape(3, 3))
    T = np.asarray(T, dtype=np.float64).reshape(3)
    t = [(Ri[i, 0] * T[0] + Ri[i, 1] * T[1]) + Ri[i, 2] * T[2] for i in range(3)]
    return Ki, Ri, t


def liftw(x, y, d, K, R, T):
    """lr_lift's formula without its rounding to float32; x, y, d float64 arrays of one shape."""
    Ki, Ri, t = _pose_inverses(K, R, T)
    with np.errstate(all="ignore"):
        xd, yd = x * d, y * d
        c = RR._rows(Ki, xd, yd, d)
        w = RR._rows(Ri, c[0], c[1], c[2])
        return [w[i] - t[i] for i in range(3)]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _under(pix, D, W):
    """Column, row and depth under each point's pixel (pix >= 0), float64."""
    D = np.asarray(D, dtype=np.float32)
    pix = np.asarray(pix, dtype=np.int64)
    return (pix % W).astype(np.float64), (pix // W).astype(np.float64), D.reshape(-1)[pix].astype(np.float64)


# ---- (a) scale sums ---------------------------------------------------------------------------------------------------------------
def scale_terms(X, valid, pix, D, K, R, T, H, W):
    """Per point: P.P, P.q, q.q (0 where the pair is left out) and whether it is used."""
    P = RR._xyz(X)
    N = P[0].shape[0]
    use = (np.asarray(valid).reshape(-1) != 0) & (np.asarray(pix) >= 0) & (np.asarray(pix) < H * W)
    x, y, d = _under(np.where(use, pix, 0), D, W)
    q = liftw(x, y, d, K, R, T)
    use = use & np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2])
    zero = np.zeros(N)
    with np.errstate(all="ignore"):
        pp, pq, qq = (np.where(use, v, zero) for v in (_dot(P, P), _dot(P, q), _dot(q, q)))
    return pp, pq, qq, use


def _tree_then_sequential(term):
    """The device's order: a tree over each workgroup's 256 terms, then the workgroup sums in index order."""
    nb = (term.shape[0] + BLOCK - 1) // BLOCK
    a = np.zeros(nb * BLOCK)
    a[:term.shape[0]] = term
    a = a.reshape(nb, BLOCK).copy()
    st = BLOCK // 2
    while st > 0:
        a[:, :st] = a[:, :st] + a[:, st:2 * st]
        st //= 2
    s = 0.0
    for b in range(nb):
        s = s + float(a[b, 0])
    return s


def scale_sums(X, valid, pix, D, K, R, T, H, W):
    """(Spp, Spq, Sqq, n) in the device's summation order."""
    pp, pq, qq, use = scale_terms(X, valid, pix, D, K, R, T, H, W)
    return _tree_then_sequential(pp), _tree_then_sequential(pq), _tree_then_sequential(qq), int(use.sum())


def fit_from_sums(spp, spq, sqq, n):
    """(scale, mse_before, mse_after): scale = spq / sqq, mse(s) = (spp - 2 s spq + s^2 sqq) / (3 n)."""
    scale = spq / sqq if n > 0 and sqq != 0.0 else 1.0
    mse = (lambda s: (spp - 2.0 * s * spq + s * s * sqq) / (3.0 * n)) if n > 0 else (lambda s: 0.0)
    return scale, mse(1.0), mse(scale)


# ---- (b) correspondences ----------------------------------------------------------------------------------------------------------
def correspond(X, pix, corr, D, K, R, T, H, W, s=1.0):
    corr = np.asarray(corr, dtype=np.int64)
    M = corr.shape[0]
    su, sv, sval = np.zeros(M + 4), np.zeros(M + 4), np.zeros(M + 4)
    su[M:], sv[M:] = [0, 0, W - 1, W - 1], [0, H - 1, 0, H - 1]
    if M == 0:
        return su, sv, sval
    _, _, _, u, v, _, _ = RR.project_points(X, K, R, T, H, W)
    P = [c[corr] for c in RR._xyz(X)]
    p_i = np.asarray(pix, dtype=np.int64)[corr]
    ok = (p_i >= 0) & (p_i < H * W)
    x, y, d = _under(np.where(ok, p_i, 0), D, W)
    w = liftw(x, y, d, K, R, T)
    _, _, t = _pose_inverses(K, R, T)
    Rm = np.asarray(R, dtype=np.float64).reshape(3, 3)
    T2 = float(np.asarray(T, dtype=np.float64).reshape(3)[2])
    rowz = lambda Xv: ((Rm[2, 0] * Xv[0] + Rm[2, 1] * Xv[1]) + Rm[2, 2] * Xv[2]) + T2
    with np.errstate(all="ignore"):
        c = [s * w[k] for k in range(3)]
        o = [-t[k] for k in range(3)]
        a = [c[k] - o[k] for k in range(3)]
        p = [P[k] - o[k] for k in range(3)]
        aa = _dot(a, a)
        tt = _dot(p, a) / aa
        m = [o[k] + a[k] * tt for k in range(3)]
        value = rowz(m) - rowz(c)
    value = np.where(ok & (aa != 0) & np.isfinite(value), value, np.nan)
    su[:M], sv[:M], sval[:M] = u[corr], v[corr], value
    return su, sv, sval


# ---- (c) scattered interpolation --------------------------------------------------------------------------------------------------
def scatter(su, sv, sval, H, W, where):
    """float32 [H,W]: the moving least squares fit at every pixel whose `where` byte is 0, 0 elsewhere."""
    where = np.asarray(where).reshape(H, W)
    out = np.zeros((H, W), dtype=np.float32)
    qy, qx = np.nonzero(where == 0)
    if qx.size == 0:
        return out
    x, y = qx.astype(np.float64), qy.astype(np.float64)
    n = x.shape[0]
    S00, S01, S02, S11, S12, S22, B0, B1, B2 = (np.zeros(n) for _ in range(9))
    vmin, vmax, used = math.inf, -math.inf, 0
    for j in range(len(sval)):
        val = float(sval[j])
        if val != val:
            continue
        dx, dy = float(su[j]) - x, float(sv[j]) - y
        d2 = (dx * dx + dy * dy) + 1e-12
        w = 1.0 / (d2 * d2)
        wx, wy, wv = w * dx, w * dy, w * val
        S00 = S00 + w
        S01 = S01 + wx
        S02 = S02 + wy
        S11 = S11 + wx * dx
        S12 = S12 + wx * dy
        S22 = S22 + wy * dy
        B0 = B0 + wv
        B1 = B1 + wv * dx
        B2 = B2 + wv * dy
        vmin, vmax = (val if val < vmin else vmin), (val if val > vmax else vmax)
        used += 1
    if not used:
        return out
    with np.errstate(all="ignore"):
        C0 = S11 * S22 - S12 * S12
        C1 = S02 * S12 - S01 * S22
        C2 = S01 * S12 - S02 * S11
        det = (S00 * C0 + S01 * C1) + S02 * C2
        num = (B0 * C0 + B1 * C1) + B2 * C2
        r = np.where(det > 1e-12 * ((S00 * S11) * S22), num / det, B0 / S00)
        r = np.where(r > vmin, r, vmin)
        r = np.where(r < vmax, r, vmax)
    out[qy, qx] = r.astype(np.float32)
    return out


def scatter_takes_fallback(su, sv, sval, H, W, where):
    """Bool per query pixel (row-major over where == 0): True where the fit is refused and Shepard's mean is taken."""
    qy, qx = np.nonzero(np.asarray(where).reshape(H, W) == 0)
    x, y = qx.astype(np.float64), qy.astype(np.float64)
    S = [np.zeros(x.shape[0]) for _ in range(6)]
    for j in range(len(sval)):
        if sval[j] != sval[j]:
            continue
        dx, dy = float(su[j]) - x, float(sv[j]) - y
        d2 = (dx * dx + dy * dy) + 1e-12
        w = 1.0 / (d2 * d2)
        wx, wy = w * dx, w * dy
        for k, v in enumerate((w, wx, wy, wx * dx, wx * dy, wy * dy)):
            S[k] = S[k] + v
    S00, S01, S02, S11, S12, S22 = S
    det = (S00 * (S11 * S22 - S12 * S12) + S01 * (S02 * S12 - S01 * S22)) + S02 * (S01 * S12 - S02 * S11)
    return ~(det > 1e-12 * ((S00 * S11) * S22))


# ---- (d) compensated lift ---------------------------------------------------------------------------------------------------------
def dream_lift(D, nd, K, R, T, s=1.0):
    D = np.asarray(D, dtype=np.float32)
    H, W = D.shape
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    dd = D.astype(np.float64).reshape(-1) + np.asarray(nd, dtype=np.float32).astype(np.float64).reshape(-1)
    w = liftw(x.reshape(-1), y.reshape(-1), dd, K, R, T)
    with np.errstate(all="ignore"):
        return np.stack([(s * w[k]).astype(np.float32) for k in range(3)], axis=0)


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
def border_corr(frame):
    """valid_idx[border_valid_idx] (R/luciddreamer.py:389-393, :414) from a restated frame: ascending cloud indices."""
    valid_idx = np.nonzero(frame["valid"])[0]
    pix = frame["pix"][valid_idx]
    return valid_idx[np.nonzero(frame["border"].reshape(-1)[pix])[0]].astype(np.int32)


def compensate(X, frame, D, K, R, T, H, W, s=1.0):
    corr = border_corr(frame)
    su, sv, sval = correspond(X, frame["pix"], corr, D, K, R, T, H, W, s)
    nd = scatter(su, sv, sval, H, W, frame["mask"])
    return dict(corr=corr, su=su, sv=sv, sval=sval, new_depth=nd, lifted=dream_lift(D, nd, K, R, T, s))


def dream_step(X, C, frame, image, D, K, R, T, H, W, scale="lstsq"):
    """(points' [3, N + n], colors' [N + n, 3], dict(scale, sums, n_corr, n_added))."""
    Xn = np.asarray(X, dtype=np.float32)
    X3 = Xn.T if Xn.shape[1] == 3 else Xn
    sums = None
    if scale == "lstsq":
        sums = scale_sums(X, frame["valid"], frame["pix"], D, K, R, T, H, W)
        s = fit_from_sums(*sums)[0]
    elif scale == "reference":
        s = 1.0
    else:
        s = float(scale)
    comp = compensate(X, frame, D, K, R, T, H, W, s)
    hole = np.nonzero(frame["mask"].reshape(-1) == 0)[0]
    image = np.asarray(image)
    cols = image.reshape(-1, 3)[hole]
    cols = cols.astype(np.float32) / 255. if image.dtype == np.uint8 else cols.astype(np.float32)
    return (np.concatenate([X3, comp["lifted"][:, hole]], axis=1), np.concatenate([np.asarray(C, dtype=np.float32), cols], axis=0),
            dict(scale=s, sums=sums, n_corr=int(comp["corr"].shape[0]), n_added=int(hole.shape[0]), comp=comp))
