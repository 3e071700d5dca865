"""References for the normals from depth and the normal losses (test helper, not collected).

  (a) torch_*: the definition by LIFTED POINTS in float64 torch -- P = d (u, v, 1), n = normalize(cross(P_S - P_N, P_E - P_W)),
      2DGS's depth_to_normal -- differentiable by autograd.  The independent reference: it shares no formula with the kernels.
  (b) closed_form / closed_form_vjp: a numpy restatement of the closed form of include/lucid_raster.h, operation by operation in
      the header's order, in a dtype of choice: float64, and float32 as the CALIBRATOR (what float32 costs on that very case).
      It returns value, count and gradient; `order` is the gather's summation order, the header's "WENS" or its reverse "SNEW".
  (c) make_case: the seeded inputs of the tests.
"""
import numpy as np
import torch


# ---- (a) float64, lifted points, autograd ---------------------------------------------------------------------------------------
def _rays(H, W, tx, ty, like):
    u = (torch.arange(W, dtype=like.dtype, device=like.device) + 0.5) * (2.0 * tx / W) - tx
    v = (torch.arange(H, dtype=like.dtype, device=like.device) + 0.5) * (2.0 * ty / H) - ty
    return u[None, :].expand(H, W), v[:, None].expand(H, W)


def torch_normals(depth, tx, ty):
    """(normals [3,H,W], valid [H,W] bool) of a depth [H,W], in its dtype (float64 for the reference) and on its device;
    differentiable.  A depth that is not > 0 is replaced by 1 before any arithmetic (its pixels are invalid anyway), so that no
    NaN reaches autograd."""
    H, W = depth.shape
    n = torch.zeros(3, H, W, dtype=depth.dtype, device=depth.device)
    valid = torch.zeros(H, W, dtype=torch.bool, device=depth.device)
    if H < 3 or W < 3:
        return n, valid
    ok = depth > 0
    d = torch.where(ok, depth, torch.ones_like(depth))
    u, v = _rays(H, W, tx, ty, depth)
    P = torch.stack([d * u, d * v, d])
    dy = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    dx = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    c = torch.cross(dy, dx, dim=0)
    m2 = (c * c).sum(0)
    inner = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[:-2, 1:-1] & ok[2:, 1:-1] & torch.isfinite(m2) & (m2 > 0)
    ni = torch.where(inner[None], c / torch.sqrt(torch.where(inner, m2, torch.ones_like(m2)))[None], torch.zeros_like(c))
    n = torch.nn.functional.pad(ni, (1, 1, 1, 1))
    valid = torch.nn.functional.pad(inner, (1, 1, 1, 1))
    return n, valid


def torch_loss(depth, tx, ty, target_normals=None, target_depth=None, pixel_weight=None, weight=1.0):
    """(loss, counted [H,W] bool) in the dtype and on the device of the tensors given (float64 on the CPU for the reference; in
    float32 on the device this is the torch composition the fused kernels replace); differentiable in depth and target_depth."""
    assert (target_normals is None) != (target_depth is None)
    H, W = depth.shape
    n, counted = torch_normals(depth, tx, ty)
    if target_depth is not None:
        t, tv = torch_normals(target_depth, tx, ty)
        counted = counted & tv
    else:
        tt = (target_normals * target_normals).sum(0)
        tv = (tt > 0) & torch.isfinite(tt)
        t = torch.where(tv[None], target_normals, torch.ones_like(target_normals)) / torch.sqrt(torch.where(tv, tt, 3 * torch.ones_like(tt)))[None]
        counted = counted & tv
    w = torch.ones(H, W, dtype=depth.dtype, device=depth.device)
    if pixel_weight is not None:
        wv = pixel_weight > 0
        w = torch.where(wv, pixel_weight, torch.zeros_like(pixel_weight))
        counted = counted & wv
    term = torch.where(counted, w * (1.0 - (n * t).sum(0)), torch.zeros(H, W, dtype=depth.dtype, device=depth.device))
    return weight * term.sum() / (H * W), counted


def reference(case, tx, ty, mode="target", with_weight=True, weight=1.0):
    """The float64 reference of one case: dict(value, count, counted, grad, grad_target (consistency mode), normals, valid)."""
    d = torch.from_numpy(case["depth"].astype(np.float64)).requires_grad_(True)
    pw = torch.from_numpy(case["pixel_weight"].astype(np.float64)) if with_weight else None
    td = tn = None
    if mode == "consistency":
        td = torch.from_numpy(case["depth_b"].astype(np.float64)).requires_grad_(True)
    else:
        tn = torch.from_numpy(case["target_normals"].astype(np.float64))
    loss, counted = torch_loss(d, tx, ty, tn, td, pw, weight)
    if loss.requires_grad:
        loss.backward()
    z = np.zeros(case["depth"].shape)
    with torch.no_grad():
        n, valid = torch_normals(d.detach(), tx, ty)
    return dict(value=float(loss.detach()), count=int(counted.sum()), counted=counted.numpy(), grad=z if d.grad is None else d.grad.numpy(),
                grad_target=None if td is None else (z if td.grad is None else td.grad.numpy()), normals=n.numpy(), valid=valid.numpy())


def reference_vjp(depth, Gn, tx, ty):
    """dL/ddepth of sum(normals * Gn) in float64 by autograd through the lifted-point definition."""
    d = torch.from_numpy(depth.astype(np.float64)).requires_grad_(True)
    n, _ = torch_normals(d, tx, ty)
    s = (n * torch.from_numpy(Gn.astype(np.float64))).sum()
    if not s.requires_grad:
        return np.zeros(depth.shape)
    s.backward()
    return np.zeros(depth.shape) if d.grad is None else d.grad.numpy()


# ---- (b) the header's closed form, in numpy, in a dtype of choice ------------------------------------------------------------------
class _Normals:
    pass


def _closed_normals(depth, tx, ty, dtype):
    """The header's normal of every pixel in `dtype`: an object with valid [H,W] and, on full-size arrays, n0 n1 n2 len u v p r gx gy
    ax ay (zeros outside the interior)."""
    f = dtype
    d = np.asarray(depth).astype(f)
    H, W = d.shape
    o = _Normals()
    o.H, o.W = H, W
    o.ax = (f(2) * f(tx)) / f(W)
    o.ay = (f(2) * f(ty)) / f(H)
    names = ("n0", "n1", "n2", "len", "u", "v", "p", "r", "gx", "gy")
    for k in names:
        setattr(o, k, np.zeros((H, W), f))
    o.valid = np.zeros((H, W), bool)
    if H < 3 or W < 3:
        return o
    with np.errstate(all="ignore"):
        x = np.arange(1, W - 1).astype(f)[None, :]
        y = np.arange(1, H - 1).astype(f)[:, None]
        u = np.broadcast_to(o.ax * (x + f(0.5)) - f(tx), (H - 2, W - 2)).astype(f)
        v = np.broadcast_to(o.ay * (y + f(0.5)) - f(ty), (H - 2, W - 2)).astype(f)
        C, E, Wd, N, S = d[1:-1, 1:-1], d[1:-1, 2:], d[1:-1, :-2], d[:-2, 1:-1], d[2:, 1:-1]
        gx, sx, gy, sy = E - Wd, E + Wd, S - N, S + N
        p, r = o.ax * sx, o.ay * sy
        a, b = r * gx, p * gy
        c2 = -((b * v + a * u) + p * r)
        m2 = (a * a + b * b) + c2 * c2
        valid = (C > 0) & (E > 0) & (Wd > 0) & (N > 0) & (S > 0) & (m2 > 0) & (m2 < np.inf)
        ln = np.sqrt(np.where(valid, m2, f(1)))
        vals = dict(n0=a / ln, n1=b / ln, n2=c2 / ln, len=ln, u=u, v=v, p=p, r=r, gx=gx, gy=gy)
    for k in names:
        getattr(o, k)[1:-1, 1:-1] = np.where(valid, vals[k], f(0))
    o.valid[1:-1, 1:-1] = valid
    assert all(getattr(o, k).dtype == f for k in names)
    return o


def closed_normals(depth, tx, ty, dtype=np.float64):
    """(normals [3,H,W], valid [H,W]) of the header's closed form in `dtype`."""
    o = _closed_normals(depth, tx, ty, dtype)
    return np.stack([o.n0, o.n1, o.n2]), o.valid


def _chain_and_gather(o, counted, G0, G1, G2, order):
    """The header's chain from G to the four neighbour terms of every pixel, and their gather in `order`."""
    f = o.n0.dtype.type
    with np.errstate(all="ignore"):
        A, B = G0 - o.u * G2, G1 - o.v * G2
        dgx, dgy = o.r * A, o.p * B
        dsx = o.ax * (o.gy * B - o.r * G2)
        dsy = o.ay * (o.gx * A - o.p * G2)
        tE, tW, tS, tN = dgx + dsx, dsx - dgx, dgy + dsy, dsy - dgy
    z = f(0)
    pad = lambda t: np.pad(np.where(counted, t, z), 1)
    tE, tW, tS, tN = pad(tE), pad(tW), pad(tS), pad(tN)
    fW, fE = tE[1:-1, :-2], tW[1:-1, 2:]               # tE of (x-1, y), tW of (x+1, y)
    fN, fS = tS[:-2, 1:-1], tN[2:, 1:-1]               # tS of (x, y-1), tN of (x, y+1)
    g = ((fW + fE) + fN) + fS if order == "WENS" else ((fS + fN) + fE) + fW
    assert order in ("WENS", "SNEW") and g.dtype == o.n0.dtype
    return g


def _loss_side(o, t0, t1, t2, counted, w, k, order):
    f = o.n0.dtype.type
    with np.errstate(all="ignore"):
        dot = (o.n0 * t0 + o.n1 * t1) + o.n2 * t2
        term = np.where(counted, w * (f(1) - dot), f(0))
        kk = (k * w) / o.len
        G0, G1, G2 = -(kk * (t0 - o.n0 * dot)), -(kk * (t1 - o.n1 * dot)), -(kk * (t2 - o.n2 * dot))
    return term, _chain_and_gather(o, counted, G0, G1, G2, order)


def closed_form(depth, tx, ty, dtype=np.float64, target_normals=None, target_depth=None, pixel_weight=None, weight=1.0,
                upstream=1.0, order="WENS"):
    """The loss of the header in `dtype` (sums in float64, as the kernels'): dict(value, count, counted, grad, grad_target,
    normals, valid)."""
    assert (target_normals is None) != (target_depth is None)
    f = dtype
    o = _closed_normals(depth, tx, ty, f)
    H, W = o.H, o.W
    counted = o.valid.copy()
    w = np.ones((H, W), f)
    if pixel_weight is not None:
        pw = np.asarray(pixel_weight).astype(f)
        with np.errstate(invalid="ignore"):
            wv = pw > 0
        w = np.where(wv, pw, f(1))
        counted &= wv
    ot = None
    if target_depth is not None:
        ot = _closed_normals(target_depth, tx, ty, f)
        counted &= ot.valid
        t0, t1, t2 = ot.n0, ot.n1, ot.n2
    else:
        a = np.asarray(target_normals).astype(f)
        with np.errstate(all="ignore"):
            tt = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
            tv = (tt > 0) & (tt < np.inf)
            tl = np.sqrt(np.where(tv, tt, f(1)))
            t0, t1, t2 = a[0] / tl, a[1] / tl, a[2] / tl
        counted &= tv
    k = (f(upstream) * f(weight)) / f(H * W)
    term, grad = _loss_side(o, t0, t1, t2, counted, w, k, order)
    total = float(term.astype(np.float64).sum())
    mean = f(total / (float(H) * float(W)))
    out = dict(value=float(f(weight) * mean), count=int(counted.sum()), counted=counted, grad=grad, grad_target=None,
               normals=np.stack([o.n0, o.n1, o.n2]), valid=o.valid)
    if ot is not None:
        out["grad_target"] = _loss_side(ot, o.n0, o.n1, o.n2, counted, w, k, order)[1]
    assert grad.dtype == f
    return out


def closed_form_vjp(depth, Gn, tx, ty, dtype=np.float64, order="WENS"):
    """dL/ddepth from Gn = dL/dnormals [3,H,W] by the header's formulas in `dtype`."""
    f = dtype
    o = _closed_normals(depth, tx, ty, f)
    g = np.asarray(Gn).astype(f)
    with np.errstate(all="ignore"):
        dn = (o.n0 * g[0] + o.n1 * g[1]) + o.n2 * g[2]
        G0, G1, G2 = (g[0] - o.n0 * dn) / o.len, (g[1] - o.n1 * dn) / o.len, (g[2] - o.n2 * dn) / o.len
    out = _chain_and_gather(o, o.valid, G0, G1, G2, order)
    assert out.dtype == f
    return out


# ---- (c) the cases -----------------------------------------------------------------------------------------------------------
TAN = (0.7, 0.45)                   # tan_fovx, tan_fovy of the kernel tests
MIN_COUNTED = 0.40                  # of the INTERIOR pixels (the only ones that can count): every non-degenerate case, asserted


def make_case(H, W, seed, kind="smooth"):
    """float32 inputs: depth [H,W] (kind "smooth": 4 + 0.8 sin(0.35 x) + 0.5 cos(0.3 y) + 0.01 randn; "rand": uniform on 0.5..10)
    with 4 % zero and 1 % NaN depths, target_normals [3,H,W] with 5 % zero vectors, pixel_weight [H,W] uniform on 0.05..1, and
    depth_b [H,W], a second surface for the consistency term (the first one warped by a few per cent, its own 2 % zeros)."""
    g = np.random.default_rng(seed)
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    if kind == "smooth":
        d = 4.0 + 0.8 * np.sin(0.35 * x) + 0.5 * np.cos(0.3 * y) + 0.01 * g.standard_normal((H, W))
    else:
        assert kind == "rand"
        d = g.uniform(0.5, 10.0, (H, W))
    clean = d.copy()
    hole = g.uniform(size=(H, W))
    d[hole < 0.04] = 0.0
    d[(hole >= 0.04) & (hole < 0.05)] = np.nan
    t = g.standard_normal((3, H, W)) + np.array([0.0, 0.0, -1.5])[:, None, None]
    t[:, g.uniform(size=(H, W)) < 0.05] = 0.0
    w = g.uniform(0.05, 1.0, (H, W))
    b = clean * (1.0 + 0.03 * np.sin(0.2 * x + 0.1 * y)) + 0.01 * g.standard_normal((H, W))
    b[g.uniform(size=(H, W)) < 0.02] = 0.0
    f = np.float32
    return dict(depth=d.astype(f), target_normals=t.astype(f), pixel_weight=w.astype(f), depth_b=b.astype(f), H=H, W=W)


def counted_fraction(ref, H, W):
    """The share of the interior pixels that count (0 when there is no interior)."""
    inner = max(H - 2, 0) * max(W - 2, 0)
    return ref["count"] / inner if inner else 0.0
