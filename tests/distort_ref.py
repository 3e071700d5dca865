"""References of the depth distortion output (lr_render_distortion / lr_distortion_backward).

Definition (include/lucid_raster.h).  For one pixel, the blend forward's walk, T = 1 at the start:
    power > 0 -> skip;  alpha = min(0.99, opacity exp(power)), alpha < 1/255 -> skip;
    test_T = T (1 - alpha), test_T < 1e-4 -> stop, not blended;  otherwise blend with w = alpha T, T = test_T.
Each blended layer has a mapped depth m = c0 + c1 z + c2 / z, and D = sum_i w_i sum_{j<i} w_j (m_i - m_j)^2.

1. render64: the float64 reference -- oracle/torch_oracle.py's pipeline restated (its lines, copied: oracle/ stays as it is) with
   the per-Gaussian depth ATTACHED and D added; autograd gives the gradient of every leaf.  The conventions of the colour path
   hold: the 0.99 clamp is differentiated as if absent, the skips, the stop and the sort order are constants.
2. walk32: the kernel's arithmetic in numpy float32 on the C oracle's stage() (tests/median_ref.walk is the model): the running
   sums A, M1, M2 of w, w mt, w mt^2 with mt = m - m_ref (the first blended layer's m), each layer's bracket held at >= 0.  It
   returns D, the layer count per pixel and a FRAGILE mask: the oracle's own fragile bits, or an alpha within a relative
   ALPHA_BAND of 1/255 on a live pixel -- there two correct float32 evaluations may blend different layers.
3. backward32: the chosen recursion of the backward (front to back: S_i = 2 D - sum_{k<=i} w_k q_k; back to front as the
   alternative) in numpy float32 on the same state, summed per Gaussian at the screen-space level (pixel-space mean, conic,
   opacity, z), against render64's autograd gradients of the same intermediates.

FWD_ERR / SHIFT_ERR hold what tests/test_distort_cpu.py measured of 2. against 1.; the GPU bars are derived from them.
"""
import functools

import numpy as np
import torch

from oracle import torch_oracle as to
from tests import helpers as hp, median_ref as mr, posed_cases as pc_

ALPHA_BAND = mr.ALPHA_BAND
FRAGILE_CAP = mr.FRAGILE_CAP
BG = mr.BG
DEGREE = mr.DEGREE
WIDE = (1000, 150, 110, 4.0)                # tests/test_gpu_median.py WIDE: Gaussians over many tiles
THIN = (40, 70, 45, 0.6)                    # few small Gaussians: pixels with 0, 1 and >= 2 layers (tests/test_distort_cpu.py)
INPUTS = dict(mr.INPUTS, wide=WIDE, thin=THIN)
POSED = "box_general"
NEAR, FAR = 0.2, 100.0
MAPS = {"ndc": (FAR / (FAR - NEAR), 0.0, -FAR * NEAR / (FAR - NEAR)), "linear": (0.0, 1.0, 0.0)}
SHIFT_PAIR = ((0.0, 1.0, 0.0), (1000.0, 1.0, 0.0))      # the linear mapping, and the same cloud pushed 1000 away in m

# Measured by tests/test_distort_cpu.py::test_float32_walk_against_float64 (`pytest -s tests/test_distort_cpu.py` prints the lines):
# max |walk32 - render64| over the non-fragile pixels, per input and mapping; the run's figure in the comment, recorded rounded up
# by at most 8 % (numpy's float32 exp is not the same bits on every CPU), and the test holds the run between 1/4 of the record
# and the record.  The GPU bar is 4 x the record: the kernel takes exp2 on scaled coefficients and contracts differently from numpy
# (the margin tests/median_ref.py gives T: T_BAND = 4 COLOR_ATOL).  Never derived from the GPU's own output.
FWD_ERR = {
    ("sparse", "ndc"): 6.5e-10,     # 6.18e-10 on D <= 3.0e-04, 30 layers at most
    ("sparse", "linear"): 1.8e-06,  # 1.63e-06 on D <= 1.33
    ("dense", "ndc"): 8.0e-11,      # 7.56e-11 on D <= 8.3e-06, 108 layers at most
    ("dense", "linear"): 8.0e-09,   # 7.61e-09 on D <= 1.06e-02
    ("small", "ndc"): 2.3e-10,      # 2.14e-10
    ("small", "linear"): 2.6e-07,   # 2.41e-07
    ("wide", "ndc"): 1.15e-10,      # 1.05e-10
    ("wide", "linear"): 1.25e-07,   # 1.17e-07
    ("thin", "ndc"): 3.8e-10,       # 3.56e-10 on D <= 2.1e-04, 4 layers at most
    ("thin", "linear"): 6.3e-07,    # 5.94e-07 on D <= 0.66
    ("posed", "ndc"): 1.05e-09,     # 9.96e-10
    ("posed", "linear"): 4.4e-06,   # 4.19e-06
}
# max |D(c0 = 0) - D(c0 = 1000)| of walk32 on "sparse", linear mapping (test_shift_pair_of_the_float32_walk: 3.10e-05 on D <= 1.33;
# without the shift the c0 = 1000 walk is off by 0.19); the GPU pair is held to 4 x this
SHIFT_ERR = 3.3e-05
# The float32 restatement of the backward (backward32, test_float32_backward_holds_the_gradient_bar) against float64 autograd at the
# screen-space level, worst tensor per input as a share of the tensor's largest entry: front to back 5.8e-06 (sparse), 1.1e-05
# (dense), 7.3e-06 (wide), 1.1e-05 (posed); back to front 5.9e-06, 1.2e-05, 7.6e-06, 1.0e-05.  Both hold GRAD_RTOL = 1e-4 with a
# factor of nine to spare, so no tensor has a bar of its own; the kernel walks front to back.


def coefficients(mapping):
    return MAPS[mapping] if isinstance(mapping, str) else tuple(float(c) for c in mapping)


# ---- 1. float64 ---------------------------------------------------------------------------------------------------------------
def render64(cloud, cam, degree, bg, coef, opacities=None, dtype=torch.float64):
    """(color [3,H,W], D [1,H,W], layers [H,W] int, inter) with autograd from the leaves of `cloud` (float64 copies that require
    grad: inter["leaves"]) to both images.  inter: the screen-space intermediates px, py, conic, op, z (retain_grad), for the
    gradient checks at that level.  opacities: a differentiable [P,1] override (anti-aliasing: the compensated opacity)."""
    tfx, tfy = hp.tan_fov(cam)
    H, W = cam.image_height, cam.image_width
    c0, c1, c2 = coef
    leaves = {k: cloud[k].detach().to(dtype).requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
    means3D, scales, rotations, shs, means2D = (leaves[k] for k in ("means3D", "scales", "rotations", "shs", "means2D"))
    op_in = leaves["opacities"] if opacities is None else opacities(leaves)
    V, Pm = cam.world_view_transform.to(dtype), cam.full_proj_transform.to(dtype)
    campos, bg = cam.camera_center.to(dtype), bg.to(dtype)
    P = means3D.shape[0]
    fx, fy = W / (2.0 * tfx), H / (2.0 * tfy)
    gx, gy = (W + 15) // 16, (H + 15) // 16

    # ---- oracle/torch_oracle.py render(), lines 72-120 ----
    p_view = means3D @ V[:3, :3] + V[3, :3]
    hom = means3D @ Pm[:3, :] + Pm[3, :]
    p_w = 1.0 / (hom[:, 3] + 0.0000001)
    ndc = hom[:, :3] * p_w[:, None]
    ndc = torch.cat([ndc[:, :2] + means2D[:, :2], ndc[:, 2:3]], dim=1)
    in_front = p_view[:, 2] > 0.2
    cov3D = to.cov3d_from_scale_rot(scales, 1.0, rotations)
    tz = p_view[:, 2]
    tz_safe = torch.where(in_front, tz, torch.ones_like(tz))
    limx, limy = 1.3 * tfx, 1.3 * tfy
    txtz, tytz = p_view[:, 0] / tz_safe, p_view[:, 1] / tz_safe
    tx = torch.where((txtz < -limx) | (txtz > limx), (txtz.clamp(-limx, limx) * tz_safe).detach(), p_view[:, 0])
    ty = torch.where((tytz < -limy) | (tytz > limy), (tytz.clamp(-limy, limy) * tz_safe).detach(), p_view[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz_safe, zero, -(fx * tx) / (tz_safe * tz_safe),
                     zero, fy / tz_safe, -(fy * ty) / (tz_safe * tz_safe)], dim=1).reshape(P, 2, 3)
    Wc = V[:3, :3].T
    A = J @ Wc
    Sig = torch.stack([cov3D[:, 0], cov3D[:, 1], cov3D[:, 2], cov3D[:, 1], cov3D[:, 3], cov3D[:, 4],
                       cov3D[:, 2], cov3D[:, 4], cov3D[:, 5]], dim=1).reshape(P, 3, 3)
    cov2 = A @ Sig @ A.transpose(1, 2)
    a, b, c = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    ok = in_front & (det != 0)
    det_s = torch.where(ok, det, torch.ones_like(det))
    conic = torch.stack([c / det_s, -b / det_s, a / det_s], dim=1)
    mid = 0.5 * (a + c)
    lam = mid + torch.sqrt(torch.clamp_min(mid * mid - det, 0.1))
    radius = torch.ceil(3.0 * torch.sqrt(lam)).detach()
    px = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5
    py = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    ri = radius.to(torch.int64).to(dtype)
    trunc = lambda t: torch.trunc(t.detach()).to(torch.int64)
    rminx = trunc((px - ri) / 16).clamp(0, gx); rmaxx = trunc((px + ri + 15) / 16).clamp(0, gx)
    rminy = trunc((py - ri) / 16).clamp(0, gy); rmaxy = trunc((py + ri + 15) / 16).clamp(0, gy)
    ok = ok & (((rmaxx - rminx) * (rmaxy - rminy)) > 0)
    d = means3D - campos[None, :]
    rgb = to.sh_to_rgb(degree, shs, d / d.norm(dim=1, keepdim=True))
    depth_g = p_view[:, 2] * 1.0                                   # ATTACHED (the oracle detaches it: its docstring (iii))
    op = op_in.reshape(-1) * 1.0
    inter = dict(px=px, py=py, conic=conic, op=op, z=depth_g, leaves=leaves)
    for k in ("px", "py", "conic", "op", "z"):
        inter[k].retain_grad()
    m_all = c0 + c1 * depth_g + c2 / torch.where(in_front, depth_g, torch.ones_like(depth_g))

    order_all = torch.argsort(depth_g.detach().to(torch.float32), stable=True)
    out_c = [[None] * gx for _ in range(gy)]
    out_d = [[None] * gx for _ in range(gy)]
    out_n = [[None] * gx for _ in range(gy)]
    for ty_ in range(gy):
        for tx_ in range(gx):
            sel = ok & (rminx <= tx_) & (tx_ < rmaxx) & (rminy <= ty_) & (ty_ < rmaxy)
            ids = order_all[sel[order_all]]
            ys, xs = torch.meshgrid(torch.arange(ty_ * 16, ty_ * 16 + 16), torch.arange(tx_ * 16, tx_ * 16 + 16), indexing="ij")
            pxf, pyf = xs.reshape(-1).to(dtype), ys.reshape(-1).to(dtype)
            if ids.numel() == 0:
                c_t = bg[:, None].expand(3, 256)
                D_t = torch.zeros(256, dtype=dtype)
                n_t = torch.zeros(256, dtype=torch.int64)
            else:
                dx = px[ids][None, :] - pxf[:, None]
                dy = py[ids][None, :] - pyf[:, None]
                cn = conic[ids]
                power = -0.5 * (cn[:, 0][None] * dx * dx + cn[:, 2][None] * dy * dy) - cn[:, 1][None] * dx * dy
                G = torch.exp(torch.clamp_max(power, 0.0))
                araw = op[ids][None, :] * G
                alpha = araw + (torch.clamp_max(araw, 0.99) - araw).detach()
                valid = (power <= 0) & (alpha.detach() >= 1.0 / 255.0)
                a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
                one_m = 1.0 - a_eff
                T_incl = torch.cumprod(one_m, dim=1)
                T_excl = torch.cat([torch.ones_like(T_incl[:, :1]), T_incl[:, :-1]], dim=1)
                stop = valid & (T_incl.detach() < 0.0001)
                done = torch.cumsum(stop.to(torch.int64), dim=1) > 0
                contrib = valid & ~done
                w = torch.where(contrib, alpha * T_excl, torch.zeros_like(alpha))
                T_fin = torch.prod(torch.where(contrib, one_m, torch.ones_like(one_m)), dim=1)
                c_t = (w @ rgb[ids]).T + T_fin[None, :] * bg[:, None]
                # ---- the distortion: D = sum_i w_i (m_i^2 A_{i-1} + M2_{i-1} - 2 m_i M1_{i-1}), prefix sums over j < i ----
                m = (m_all[ids] - m_all[ids].detach().min())[None, :]            # (a constant shift: float64 needs none)
                wm, wmm = w * m, w * m * m
                A_prev = torch.cumsum(w, dim=1) - w
                M1_prev = torch.cumsum(wm, dim=1) - wm
                M2_prev = torch.cumsum(wmm, dim=1) - wmm
                D_t = (w * (m * m * A_prev + M2_prev - 2.0 * m * M1_prev)).sum(dim=1)
                n_t = contrib.sum(dim=1)
            out_c[ty_][tx_] = c_t.reshape(3, 16, 16)
            out_d[ty_][tx_] = D_t.reshape(1, 16, 16)
            out_n[ty_][tx_] = n_t.reshape(16, 16)
    color = torch.cat([torch.cat(row, dim=2) for row in out_c], dim=1)[:, :H, :W]
    D = torch.cat([torch.cat(row, dim=2) for row in out_d], dim=1)[:, :H, :W]
    layers = torch.cat([torch.cat(row, dim=1) for row in out_n], dim=0)[:H, :W]
    return color, D, layers, inter


def grads64(cloud, cam, degree, bg, coef, G, gc=None, opacities=None):
    """{leaf: float64 gradient} and {intermediate: gradient} of <G, D> (+ <gc, color>) from render64."""
    color, D, layers, inter = render64(cloud, cam, degree, bg, coef, opacities=opacities)
    loss = (D * torch.as_tensor(G, dtype=D.dtype)).sum()
    if gc is not None:
        loss = loss + (color * gc.to(D.dtype)).sum()
    loss.backward()
    L = inter["leaves"]
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    leaf = dict(means3D=z(L["means3D"]), means2D=z(L["means2D"]), opacity=z(L["opacities"]), scales=z(L["scales"]),
                rotations=z(L["rotations"]), sh=z(L["shs"]))
    mid = {k: z(inter[k]) for k in ("px", "py", "conic", "op", "z")}
    return leaf, mid, D.detach().numpy()[0], layers.numpy()


# ---- 2. float32 walk ----------------------------------------------------------------------------------------------------------
def _tiles(st, W, H):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    for tile in range(gx * gy):
        tx, ty = tile % gx, tile // gx
        ys, xs = np.mgrid[ty * 16:min(H, ty * 16 + 16), tx * 16:min(W, tx * 16 + 16)]
        r0, r1 = (int(v) for v in st["ranges"][tile])
        yield ys.ravel(), xs.ravel(), r0, r1


def _alpha32(st, g, pxf, pyf):
    f32 = np.float32
    m2, co = st["means2D"], st["conic_opacity"]
    dx, dy = m2[g, 0] - pxf, m2[g, 1] - pyf
    a, b, c, op = (f32(v) for v in co[g])
    power = f32(-0.5) * (a * dx * dx + c * dy * dy) - b * dx * dy
    with np.errstate(over="ignore"):
        t = op * np.exp(power)                                       # alpha before the clamp
    return dx, dy, power, t


def _map32(coef, z):
    f32 = np.float32
    c0, c1, c2 = (f32(c) for c in coef)
    with np.errstate(divide="ignore", invalid="ignore"):             # (depth 0: a Gaussian that was never listed)
        return (c0 + c1 * z) + c2 / z                                    # csrc/render_distort.hip dst_map


def walk32(st, W, H, coef, shift=True):
    """(D [H,W] float32, layers [H,W] int32, fragile [H,W] bool, moments [H,W,4] float32) from an oracle result's stage()."""
    f32 = np.float32
    D = np.zeros((H, W), f32)
    layers = np.zeros((H, W), np.int32)
    mom = np.zeros((H, W, 4), f32)
    fragile = st["fragile"] != 0
    plist = st["point_list"]
    thr = f32(1.0) / f32(255.0)
    mz = _map32(coef, st["depths"].astype(f32))
    for ys, xs, r0, r1 in _tiles(st, W, H):
        pxf, pyf = xs.astype(f32), ys.astype(f32)
        n = xs.size
        T = np.ones(n, f32)
        A, M1, M2, Dp, mref = (np.zeros(n, f32) for _ in range(5))
        cnt = np.zeros(n, np.int32)
        active = np.ones(n, bool)
        frag = np.zeros(n, bool)
        for k in range(r0, r1):
            if not active.any():
                break
            g = int(plist[k])
            _, _, power, t = _alpha32(st, g, pxf, pyf)
            ok = power <= 0
            alpha = np.minimum(f32(0.99), t)
            frag |= active & ok & (np.abs(alpha.astype(np.float64) - 1.0 / 255.0) <= ALPHA_BAND / 255.0)
            use = active & ok & (alpha >= thr)
            test_T = T * (f32(1.0) - alpha)
            stop = use & (test_T < f32(0.0001))
            blend = use & ~stop
            w = alpha * T
            first = blend & (cnt == 0)
            mref = np.where(first & shift, mz[g], mref)
            mt = mz[g] - mref
            q = np.maximum(f32(0), mt * (mt * A - f32(2) * M1) + M2)
            Dp = np.where(blend, Dp + w * q, Dp)
            A = np.where(blend, A + w, A)
            M1 = np.where(blend, M1 + w * mt, M1)
            M2 = np.where(blend, M2 + (w * mt) * mt, M2)
            T = np.where(blend, test_T, T)
            cnt += blend
            active &= ~stop
        D[ys, xs] = Dp
        layers[ys, xs] = cnt
        mom[ys, xs] = np.stack([A, M1, M2, mref], axis=1)
        fragile[ys, xs] |= frag
    return D, layers, fragile, mom


# ---- 3. float32 backward ------------------------------------------------------------------------------------------------------
def backward32(st, W, H, coef, G, D, mom, P, direction="front"):
    """Screen-space gradients {px, py, conic [P,3], op, z} (float32 sums, pixel units) of <G, D> by the kernel's recursion:
    dD/dalpha_i = T_i q_i - S_i / (1 - alpha_i) with S_i = 2 D - sum_{k<=i} w_k q_k ("front") or the suffix sum ("back")."""
    f32 = np.float32
    c0, c1, c2 = (f32(c) for c in coef)
    out = dict(px=np.zeros(P, f32), py=np.zeros(P, f32), conic=np.zeros((P, 3), f32), op=np.zeros(P, f32), z=np.zeros(P, f32))
    plist, co = st["point_list"], st["conic_opacity"]
    thr = f32(1.0) / f32(255.0)
    zs = st["depths"].astype(f32)
    mz = _map32(coef, zs)
    G = np.asarray(G, f32).reshape(H, W)
    for ys, xs, r0, r1 in _tiles(st, W, H):
        pxf, pyf = xs.astype(f32), ys.astype(f32)
        n = xs.size
        g_up, D2 = G[ys, xs], f32(2) * D[ys, xs]
        A, M1, M2, mref = (mom[ys, xs, i] for i in range(4))
        T = np.ones(n, f32)
        active = np.ones(n, bool)
        steps = []                                                   # (g, blend, t, alpha, T before, w, q, mt, dx, dy)
        for k in range(r0, r1):
            if not active.any():
                break
            g = int(plist[k])
            dx, dy, power, t = _alpha32(st, g, pxf, pyf)
            alpha = np.minimum(f32(0.99), t)
            use = active & (power <= 0) & (alpha >= thr)
            test_T = T * (f32(1.0) - alpha)
            stop = use & (test_T < f32(0.0001))
            blend = use & ~stop
            al = np.where(blend, alpha, f32(0))
            mt = mz[g] - mref
            q = mt * (mt * A - f32(2) * M1) + M2
            steps.append((g, blend, np.where(blend, t, f32(0)), al, T.copy(), al * T, q, mt, dx, dy))
            T = np.where(blend, test_T, T)
            active &= ~stop
        if direction == "front":
            C = np.zeros(n, f32)
            S_of = []
            for (_, _, _, _, _, w, q, _, _, _) in steps:
                C = C + w * q
                S_of.append(D2 - C)
        else:
            S = np.zeros(n, f32)
            S_of = [None] * len(steps)
            for i in range(len(steps) - 1, -1, -1):
                S_of[i] = S
                S = S + steps[i][5] * steps[i][6]
        for (g, blend, tm, al, Tb, w, q, mt, dx, dy), S in zip(steps, S_of):
            if not blend.any():
                continue
            dDda = Tb * q - S / (f32(1) - al)
            dop = tm * (g_up * dDda)                                 # opacity x G x dL/dalpha; 0 where not blended
            a, b, c, o = (f32(v) for v in co[g])
            # dG/dmean = G (-a dx - b dy, -c dy - b dx); dG/dconic = G (-0.5 dx^2, -dx dy, -0.5 dy^2)
            out["px"][g] += (dop * (-a * dx - b * dy)).sum(dtype=f32)
            out["py"][g] += (dop * (-c * dy - b * dx)).sum(dtype=f32)
            out["conic"][g] += np.array([(f32(-0.5) * dop * dx * dx).sum(dtype=f32), (-dop * dx * dy).sum(dtype=f32),
                                         (f32(-0.5) * dop * dy * dy).sum(dtype=f32)], f32)
            out["op"][g] += (dop.sum(dtype=f32) / o) if o > 0 else f32(0)
            out["z"][g] += ((f32(2) * w) * ((mt * A - M1) * g_up)).sum(dtype=f32) * (c1 - c2 / (zs[g] * zs[g]))
    return out


# ---- inputs and shared references ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """(cam, cloud, degree, bg) of an input: the box inputs of INPUTS, or "posed"."""
    if name == "posed":
        cam, cloud, degree = pc_.make(POSED)
        return cam, cloud, degree, torch.tensor(pc_.BG)
    P, W, H, s = INPUTS[name]
    cam, cloud = hp.box_setup(P, W, H, seed=0, scale_mult=s)
    return cam, cloud, DEGREE, torch.tensor(BG)


@functools.lru_cache(maxsize=None)
def stage(name):
    cam, cloud, degree, bg = case(name)
    ref = hp.run_oracle(cloud, cam, degree, bg)
    return ref, ref["res"].stage()


def upstream(H, W, fragile=None, seed=37):
    """Seeded upstream of D, |G| in [0.5, 1.5) with random signs, zero on the fragile pixels."""
    g = torch.Generator().manual_seed(seed)
    G = ((0.5 + torch.rand(1, H, W, generator=g)) * (1.0 - 2.0 * torch.randint(0, 2, (1, H, W), generator=g))).float()
    if fragile is not None:
        G[0][torch.from_numpy(np.ascontiguousarray(fragile))] = 0.0
    return G


@functools.lru_cache(maxsize=None)
def reference(name, mapping):
    """dict(D64, layers64, D32, layers32, fragile, mom32, G, leaf, mid): both references of an input and mapping, the seeded
    upstream (zero on fragile pixels) and render64's gradients of <G, D>; computed once, shared, read-only."""
    cam, cloud, degree, bg = case(name)
    H, W = cam.image_height, cam.image_width
    coef = coefficients(mapping)
    _, st = stage(name)
    D32, layers32, fragile, mom32 = walk32(st, W, H, coef)
    G = upstream(H, W, fragile)
    leaf, mid, D64, layers64 = grads64(cloud, cam, degree, bg, coef, G.numpy())
    out = dict(D64=D64, layers64=layers64, D32=D32, layers32=layers32, fragile=fragile, mom32=mom32, G=G, leaf=leaf, mid=mid)
    for v in list(leaf.values()) + list(mid.values()) + [D64, layers64, D32, layers32, fragile, mom32]:
        v.setflags(write=False)
    return out


def raw_grads(cloud, leaf):
    """The gradients of the STORED parameters (log-scales, logit-opacities, quaternions before normalisation: what
    gaussian_renderer.GaussianCloud keeps of `cloud`) from the activated leaves' float64 gradients, by the chain rule."""
    s = cloud["scales"].double().numpy()
    o = cloud["opacities"].double().numpy().clip(1e-6, 1 - 1e-6)
    r = cloud["rotations"].double().numpy()
    n = np.linalg.norm(r, axis=1, keepdims=True)
    q = r / n
    g = leaf["rotations"]
    return dict(xyz=leaf["means3D"], means2D=leaf["means2D"], opacity=leaf["opacity"] * o * (1 - o), scaling=leaf["scales"] * s,
                rotation=(g - q * (q * g).sum(axis=1, keepdims=True)) / n)


@functools.lru_cache(maxsize=None)
def aa_reference(name, mapping):
    """reference() under anti-aliasing: the blend sees opacity * coef (tests/aa_ref.py) -- the float32 walk on the C oracle's state
    of the pre-scaled cloud (coef32), the float64 gradients through coef64.  dict(D64, fragile, G, leaf)."""
    from tests import aa_ref
    cam, cloud, degree, bg = case(name)
    H, W = cam.image_height, cam.image_width
    tfx, tfy = hp.tan_fov(cam)
    coef = coefficients(mapping)
    c32 = aa_ref.coef32(cloud["means3D"], cam.world_view_transform, tfx, tfy, W, H, cloud["scales"], cloud["rotations"])
    pre = dict(cloud, opacities=(cloud["opacities"] * torch.from_numpy(np.asarray(c32, np.float32))[:, None]).contiguous())
    st = hp.run_oracle(pre, cam, degree, bg)["res"].stage()
    _, _, fragile, _ = walk32(st, W, H, coef)
    G = upstream(H, W, fragile)
    comp = lambda L: L["opacities"] * aa_ref.coef64(L["means3D"], cam.world_view_transform, tfx, tfy, W, H, L["scales"],
                                                     L["rotations"])[:, None]
    leaf, _, D64, _ = grads64(cloud, cam, degree, bg, coef, G.numpy(), opacities=comp)
    return dict(D64=D64, fragile=fragile, G=G, leaf=leaf)
