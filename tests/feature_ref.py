"""References of the N-channel feature map output (lr_render_features / lr_render_features_backward).

Definition (include/lucid_raster.h).  features [P,C] float32, used as given.  Per pixel: F[c] = sum_i w_i f_i[c] over the layers
the blend forward applied, w_i = alpha_i T_i with the forward's skips, 0.99 clamp and 1e-4 stop; no background, no normalisation.

1. render64: the float64 definition is literally the workaround the pass replaces: oracle.torch_oracle.render with
   colors_precomp = features[:, 3k:3k+3] (zero-padded to three columns), background 0, dtype float64, once per group of three
   channels, with autograd to every leaf and to `features`.
2. walk32: the kernel's arithmetic in numpy float32 on the C oracle's stage(), with distort_ref's fragile mask: the decisions are
   the distortion walk's.
3. backward32: the front-to-back recursion dL/dalpha_i = T_i c_i - (F.g - sum_{k<=i} w_k c_k) / (1 - alpha_i), c_i = f_i . g, in
   numpy float32, summed at the screen-space level (pixel-space mean, conic, opacity) plus dL/df per Gaussian; screen64 is its
   float64 autograd partner on the same staged values and lists.

One seeded table of C_MAX channels per input serves every channel count: a smaller C takes its first columns, so the references
are computed once at C_MAX and sliced (a channel's value does not depend on its neighbours).
FWD_ERR holds what tests/test_features_cpu.py measured of 2. against 1.; the GPU bar is 4 x it.
"""
import functools

import numpy as np
import torch

from oracle import torch_oracle as to
from tests import distort_ref as dr, helpers as hp

FRAGILE_CAP = dr.FRAGILE_CAP
K = 16                                  # the shipped chunk width (csrc/render_features.hip FTR_K; asserted on the CPU)
CHANNELS = (1, 3, 5, K, K + 3, 2 * K + 1)   # the minimum, the colour path's width, a lone partial chunk, a full chunk, full + tail,
C_MAX = max(CHANNELS)                       # two full + tail
NAMES = ("sparse", "dense", "wide", "thin", "posed")

# Measured by tests/test_features_cpu.py::test_float32_walk_against_float64 (`pytest -s` prints the lines): max |walk32 -
# render64| over the C_MAX planes of the non-fragile pixels, per input; the run's figure in the comment, recorded rounded up by at
# most 8 % (numpy's float32 exp is not the same bits on every CPU), and the test holds the run between 1/4 of the record and the
# record.  The GPU bar is 4 x the record (render_normals_ref.FWD_ERR's margin).  Never derived from the GPU's own output.
FWD_ERR = {
    "sparse": 3.2e-06,      # 2.979e-06 on |F| <= 0.951, 30 layers at most
    "dense": 6.5e-07,       # 6.060e-07 on |F| <= 0.943, 108 layers at most
    "wide": 6.7e-07,        # 6.236e-07, 104 layers at most
    "thin": 5.9e-07,        # 5.525e-07, 4 layers at most
    "posed": 5.8e-06,       # 5.435e-06
}

case = dr.case
stage = dr.stage
raw_grads = dr.raw_grads


def features_of(name, C=C_MAX, seed=53):
    """The input's seeded table [P,C] float32, |f| <= 1: the first C columns of its C_MAX-column table."""
    P = case(name)[1]["means3D"].shape[0]
    g = torch.Generator().manual_seed(seed + sum(map(ord, name)))
    return (2.0 * torch.rand(P, C_MAX, generator=g) - 1.0).float()[:, :C].contiguous()


def upstream(C, H, W, fragile=None, seed=59):
    """Seeded upstream of F [C,H,W], |G| in [0.5, 1.5) with random signs, zero on the fragile pixels; the first C planes of the
    C_MAX-plane draw."""
    g = torch.Generator().manual_seed(seed)
    G = ((0.5 + torch.rand(C_MAX, H, W, generator=g)) * (1.0 - 2.0 * torch.randint(0, 2, (C_MAX, H, W), generator=g))).float()
    if fragile is not None:
        G[:, torch.from_numpy(np.ascontiguousarray(fragile))] = 0.0
    return G[:C].contiguous()


# ---- 1. float64: the workaround ---------------------------------------------------------------------------------------------------
def render64(cloud, cam, feats, opacities=None, cov3D=None):
    """(F [C,H,W] float64, leaves) with autograd from `leaves` (float64 copies of the cloud's tensors that require grad, means2D,
    "features", and with cov3D (a [P,6] tensor) "cov3D" in place of scales + rotations) to F: ceil(C/3) renders of oracle.torch_oracle.render
    with colors_precomp = three columns of the table and background 0.  opacities: a differentiable [P,1] override from the
    leaves (anti-aliasing)."""
    dtype = torch.float64
    tfx, tfy = hp.tan_fov(cam)
    H, W = cam.image_height, cam.image_width
    leaves = {k: cloud[k].detach().to(dtype).requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
    leaves["features"] = feats.detach().to(dtype).requires_grad_(True)
    geo = dict(scales=leaves["scales"], rotations=leaves["rotations"])
    if cov3D is not None:
        leaves["cov3D"] = cov3D.detach().to(dtype).requires_grad_(True)
        geo = dict(cov3D_precomp=leaves["cov3D"])
    op_in = leaves["opacities"] if opacities is None else opacities(leaves)
    f = leaves["features"]
    C = f.shape[1]
    planes = []
    for k in range(0, C, 3):
        cols = f[:, k:k + 3]
        if cols.shape[1] < 3:
            cols = torch.cat([cols, torch.zeros(cols.shape[0], 3 - cols.shape[1], dtype=dtype)], dim=1)
        color, _, _ = to.render(leaves["means3D"], op_in, cam.world_view_transform, cam.full_proj_transform, cam.camera_center,
                                tfx, tfy, H, W, torch.zeros(3), colors_precomp=cols, means2D=leaves["means2D"], dtype=dtype, **geo)
        planes.append(color[:min(3, C - k)])
    return torch.cat(planes, dim=0), leaves


def grads64(cloud, cam, feats, G, opacities=None, cov3D=None):
    """({leaf: float64 gradient of <G, F>}, F64) from render64; the leaf names are the operator's."""
    F, L = render64(cloud, cam, feats, opacities=opacities, cov3D=cov3D)
    (F * torch.as_tensor(np.asarray(G), dtype=F.dtype)).sum().backward()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    leaf = dict(means3D=z(L["means3D"]), means2D=z(L["means2D"]), opacity=z(L["opacities"]), scales=z(L["scales"]),
                rotations=z(L["rotations"]), features=z(L["features"]))
    if cov3D is not None:
        leaf["cov3D"] = z(L["cov3D"])
    return leaf, F.detach().numpy()


# ---- 2. float32 walk --------------------------------------------------------------------------------------------------------------
def walk32(st, W, H, feats):
    """(F [C,H,W] float32, layers [H,W] int32, fragile [H,W] bool) from an oracle result's stage() and the table [P,C]."""
    f32 = np.float32
    feats = np.asarray(feats, f32)
    C = feats.shape[1]
    F = np.zeros((C, H, W), f32)
    layers = np.zeros((H, W), np.int32)
    fragile = st["fragile"] != 0
    plist = st["point_list"]
    thr = f32(1.0) / f32(255.0)
    for ys, xs, r0, r1 in dr._tiles(st, W, H):
        pxf, pyf = xs.astype(f32), ys.astype(f32)
        n = xs.size
        T = np.ones(n, f32)
        acc = np.zeros((C, n), f32)
        cnt = np.zeros(n, np.int32)
        active = np.ones(n, bool)
        frag = np.zeros(n, bool)
        for k in range(r0, r1):
            if not active.any():
                break
            g = int(plist[k])
            _, _, power, t = dr._alpha32(st, g, pxf, pyf)
            ok = power <= 0
            alpha = np.minimum(f32(0.99), t)
            frag |= active & ok & (np.abs(alpha.astype(np.float64) - 1.0 / 255.0) <= dr.ALPHA_BAND / 255.0)
            use = active & ok & (alpha >= thr)
            test_T = T * (f32(1.0) - alpha)
            stop = use & (test_T < f32(0.0001))
            blend = use & ~stop
            w = np.where(blend, alpha * T, f32(0))
            acc = acc + w[None, :] * feats[g][:, None]               # every channel a chain of its own, in list order
            T = np.where(blend, test_T, T)
            cnt += blend
            active &= ~stop
        F[:, ys, xs] = acc
        layers[ys, xs] = cnt
        fragile[ys, xs] |= frag
    return F, layers, fragile


# ---- 3. float32 backward, and its float64 partner -----------------------------------------------------------------------------------
def backward32(st, W, H, feats, G, F, P):
    """Screen-space gradients {px, py, conic [P,3], op, f [P,C]} (float32 sums, pixel units) of <G, F> by the kernel's recursion,
    front to back: dL/dalpha_i = T_i c_i - (F.g - sum_{k<=i} w_k c_k) / (1 - alpha_i), c_i = f_i . g."""
    f32 = np.float32
    feats = np.asarray(feats, f32)
    C = feats.shape[1]
    out = dict(px=np.zeros(P, f32), py=np.zeros(P, f32), conic=np.zeros((P, 3), f32), op=np.zeros(P, f32), f=np.zeros((P, C), f32))
    plist, co = st["point_list"], st["conic_opacity"]
    thr = f32(1.0) / f32(255.0)
    G = np.asarray(G, f32).reshape(C, H, W)
    for ys, xs, r0, r1 in dr._tiles(st, W, H):
        pxf, pyf = xs.astype(f32), ys.astype(f32)
        n = xs.size
        g_up = G[:, ys, xs]
        Fg = np.zeros(n, f32)
        for c in range(C):
            Fg = Fg + F[c, ys, xs] * g_up[c]
        T = np.ones(n, f32)
        Cs = np.zeros(n, f32)
        active = np.ones(n, bool)
        for k in range(r0, r1):
            if not active.any():
                break
            g = int(plist[k])
            dx, dy, power, t = dr._alpha32(st, g, pxf, pyf)
            alpha_f = np.minimum(f32(0.99), t)
            use = active & (power <= 0) & (alpha_f >= thr)
            test_T = T * (f32(1.0) - alpha_f)
            stop = use & (test_T < f32(0.0001))
            blend = use & ~stop
            active &= ~stop
            if not blend.any():
                continue
            tm = np.where(blend, t, f32(0))
            al = np.minimum(f32(0.99), tm)
            w = al * T
            c_i = np.zeros(n, f32)
            for c in range(C):
                c_i = c_i + feats[g, c] * g_up[c]
            Cs = Cs + w * c_i
            dFda = T * c_i - (Fg - Cs) / (f32(1) - al)
            dop = tm * dFda                                          # opacity x G x dL/dalpha; 0 where not blended
            T = np.where(blend, test_T, T)
            a, b, cc, o = (f32(v) for v in co[g])
            out["px"][g] += (dop * (-a * dx - b * dy)).sum(dtype=f32)
            out["py"][g] += (dop * (-cc * dy - b * dx)).sum(dtype=f32)
            out["conic"][g] += np.array([(f32(-0.5) * dop * dx * dx).sum(dtype=f32), (-dop * dx * dy).sum(dtype=f32),
                                         (f32(-0.5) * dop * dy * dy).sum(dtype=f32)], f32)
            out["op"][g] += (dop.sum(dtype=f32) / o) if o > 0 else f32(0)
            out["f"][g] += (w[None, :] * g_up).sum(axis=1, dtype=f32)
    return out


def screen64(st, W, H, feats, G):
    """The same gradients {px, py, conic, op, f} by float64 autograd: the staged float32 means, conics and opacities as float64
    leaves, the oracle's own tile lists, the blend of oracle.torch_oracle.render's tile loop with the table's C columns."""
    dt = torch.float64
    m2, co = torch.from_numpy(np.asarray(st["means2D"], np.float64)), torch.from_numpy(np.asarray(st["conic_opacity"], np.float64))
    px, py = m2[:, 0].clone().requires_grad_(True), m2[:, 1].clone().requires_grad_(True)
    conic, op = co[:, :3].clone().requires_grad_(True), co[:, 3].clone().requires_grad_(True)
    f = torch.as_tensor(np.asarray(feats), dtype=dt).clone().requires_grad_(True)
    Gt = torch.as_tensor(np.asarray(G), dtype=dt)
    plist = np.asarray(st["point_list"]).astype(np.int64)
    loss = torch.zeros((), dtype=dt)
    for ys, xs, r0, r1 in dr._tiles(st, W, H):
        if r1 <= r0:
            continue
        ids = torch.from_numpy(plist[r0:r1])
        pxf, pyf = torch.from_numpy(xs.astype(np.float64)), torch.from_numpy(ys.astype(np.float64))
        dx = px[ids][None, :] - pxf[:, None]
        dy = py[ids][None, :] - pyf[:, None]
        cn = conic[ids]
        power = -0.5 * (cn[:, 0][None] * dx * dx + cn[:, 2][None] * dy * dy) - cn[:, 1][None] * dx * dy
        araw = op[ids][None, :] * torch.exp(torch.clamp_max(power, 0.0))
        alpha = araw + (torch.clamp_max(araw, 0.99) - araw).detach()
        valid = (power <= 0) & (alpha.detach() >= 1.0 / 255.0)
        one_m = 1.0 - torch.where(valid, alpha, torch.zeros_like(alpha))
        T_incl = torch.cumprod(one_m, dim=1)
        T_excl = torch.cat([torch.ones_like(T_incl[:, :1]), T_incl[:, :-1]], dim=1)
        done = torch.cumsum((valid & (T_incl.detach() < 0.0001)).to(torch.int64), dim=1) > 0
        w = torch.where(valid & ~done, alpha * T_excl, torch.zeros_like(alpha))
        loss = loss + ((w @ f[ids]) * Gt[:, torch.from_numpy(ys), torch.from_numpy(xs)].T).sum()
    loss.backward()
    z = lambda t: t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))
    return dict(px=z(px), py=z(py), conic=z(conic), op=z(op), f=z(f))


# ---- shared references --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(feats, F64, F32, layers32, fragile, G, leaf, visible) at C_MAX channels: both references of an input, the seeded
    upstream (zero on fragile pixels) and render64's gradients of <G, F>; computed once, shared, read-only.  A smaller C reads
    feats[:, :C] and F64[:C]; the gradients are C_MAX's."""
    cam, cloud, _, _ = case(name)
    H, W = cam.image_height, cam.image_width
    ref, st = stage(name)
    feats = features_of(name)
    F32, layers32, fragile = walk32(st, W, H, feats.numpy())
    G = upstream(C_MAX, H, W, fragile)
    leaf, F64 = grads64(cloud, cam, feats, G.numpy())
    out = dict(feats=feats, F64=F64, F32=F32, layers32=layers32, fragile=fragile, G=G, leaf=leaf,
               visible=np.asarray(ref["radii"]) > 0)
    for v in list(leaf.values()) + [F64, F32, layers32, fragile]:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def aa_reference(name):
    """reference() under anti-aliasing, as distort_ref.aa_reference: dict(feats, F64, fragile, G, leaf)."""
    from tests import aa_ref
    cam, cloud, degree, bg = case(name)
    H, W = cam.image_height, cam.image_width
    tfx, tfy = hp.tan_fov(cam)
    c32 = aa_ref.coef32(cloud["means3D"], cam.world_view_transform, tfx, tfy, W, H, cloud["scales"], cloud["rotations"])
    pre = dict(cloud, opacities=(cloud["opacities"] * torch.from_numpy(np.asarray(c32, np.float32))[:, None]).contiguous())
    st = hp.run_oracle(pre, cam, degree, bg)["res"].stage()
    feats = features_of(name)
    _, _, fragile = walk32(st, W, H, feats.numpy())
    G = upstream(C_MAX, H, W, fragile)
    comp = lambda L: L["opacities"] * aa_ref.coef64(L["means3D"], cam.world_view_transform, tfx, tfy, W, H, L["scales"],
                                                     L["rotations"])[:, None]
    leaf, F64 = grads64(cloud, cam, feats, G.numpy(), opacities=comp)
    return dict(feats=feats, F64=F64, fragile=fragile, G=G, leaf=leaf)


@functools.lru_cache(maxsize=None)
def cov_reference(name):
    """dict(cov3D float32 [P,6], leaf) for the input given by cov3D_precomp = the covariance of its scales and rotations: the
    gradients of <G, F> with reference(name)'s table and upstream, "cov3D" among them."""
    cam, cloud, _, _ = case(name)
    r = reference(name)
    cov = to.cov3d_from_scale_rot(cloud["scales"].double(), 1.0, cloud["rotations"].double()).float().contiguous()
    leaf, _ = grads64(cloud, cam, r["feats"], r["G"].numpy(), cov3D=cov)
    return dict(cov3D=cov, leaf=leaf)
