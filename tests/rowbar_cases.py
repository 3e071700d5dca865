"""Seeded cases of the per-row gradient bar (test helper, not collected), shared by tests/test_rowbar_cpu.py -- which checks on
the CPU that the references alone stay inside the bar on every case, with no row excused -- and tests/test_gpu_rowbar.py.

Every case is small enough that the float64 torch oracle runs in well under a second (P <= 400, images <= 96 x 80) and names the
term or the class of rows it is there for:

  sparse_deg0..3     box cloud, one run per SH degree.  Degree 0 has no view-direction term: the covariance-through-J term of
                     dL/dmeans3D is the only small one left.
  occluded           scale_mult = 3: rows hidden behind others, 1e-4 of the tensor maximum and below.
  posed              translated, pitched and rolled camera (posed_cases "general") on a ragged 77 x 53 image: every entry of the
                     view matrix is used in the position gradient.
  fov_clamp          large Gaussians beyond 1.3 tan(fov/2) in x only and in y only (x_grad_mul / y_grad_mul), as tests/ref_cases.py.
  sh_clamp           colours clamped at 0: the `clamped` mask zeroes the gradient per channel.  Ragged 72 x 56.
  precomp            cov3D_precomp with colors_precomp: the dL/dcov3D and dL/dcolor rows.
  scale_modifier     scale_modifier = 1.7 on scales and rotations.
  long_lists         400 large splats on 2 x 2 tiles: every tile's list is longer than the 256 entries of a segment of the blend
                     backward (common.h BWD_SEG), so the segmented and the whole-list walks differ; most rows are deep in the list.
  constant_upstream  dL/dpixel = 1 everywhere, every splat wholly on screen: the position terms nearly cancel by symmetry and what
                     remains of dL/dmeans3D is the small terms -- the worst conditioning, where the calibrators matter.

References: float64 autograd through oracle/torch_oracle.render (tests/grad_oracle.render where depth or alpha carry a gradient);
calibrators: the same in float32 and, where the mode has one, the C oracle.  Computed once per process (functools.lru_cache);
callers do not modify them."""
import functools

import numpy as np
import torch

from luciddreamer_amd import cameras, synthetic
from oracle import torch_oracle
from tests import aa_ref, grad_oracle, helpers as hp, posed_cases as pc, ref_cases

BG = (0.1, 0.3, 0.7)
NAMES_SH = ("means2D", "opacity", "means3D", "scales", "rotations", "sh")
NAMES_PRE = ("means2D", "opacity", "means3D", "cov3D", "colors")
RAW_NAMES = ("means2D", "_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")

# The first seeds (from 1) at which the C oracle, judged as if it were the kernel with the float32 torch run as its only
# calibrator, and the float32 torch run judged against the C oracle, need no excuse in any tensor, and at which the case has the
# rows it is there for (tests/test_rowbar_cpu.py asserts both).
SEEDS = {"sparse_deg0": 1, "sparse_deg1": 1, "sparse_deg2": 1, "sparse_deg3": 1, "occluded": 1, "posed": 6, "fov_clamp": 2,
         "sh_clamp": 3, "precomp": 1, "scale_modifier": 1, "long_lists": 1, "constant_upstream": 1}
NAMES = tuple(SEEDS)

# the multi-view step: three views of `occluded`, the identity camera and two posed ones (yaw, pitch, roll, translation) that both
# look past one side of the cloud, so that a third of the rows is visible in the first view only
VIEW_POSES = ((0.0, 0.0, 0.0, (0.0, 0.0, 0.0)), (0.25, -0.1, 0.3, (0.9, -0.3, 0.4)), (0.35, 0.1, -0.2, (1.3, 0.3, 0.3)))
VIEW_CASE = "occluded"


def _t(cloud_np):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cloud_np.items()}


def _on_screen_cloud(P, W, H, seed):
    """P splats of 1.2 - 2.5 px (standard deviation on the screen) whose centres keep 20 px from every edge: wholly on screen,
    several layers deep."""
    g = torch.Generator().manual_seed(seed)
    cam = cameras.identity_camera(W, H)
    tfx, tfy = hp.tan_fov(cam)
    px = 2.0 * tfx / W
    z = 2.0 + 3.0 * torch.rand(P, generator=g)
    cx = 20.0 + (W - 40.0) * torch.rand(P, generator=g)
    cy = 20.0 + (H - 40.0) * torch.rand(P, generator=g)
    x = ((2.0 * cx + 1.0) / W - 1.0) * tfx * z
    y = ((2.0 * cy + 1.0) / H - 1.0) * tfy * z
    s = (1.2 + 1.3 * torch.rand(P, 1, generator=g)) * px * z[:, None] * torch.exp(0.2 * torch.randn(P, 3, generator=g))
    q = torch.randn(P, 4, generator=g)
    shs = torch.empty(P, 16, 3)
    shs[:, 0, :] = (torch.rand(P, 3, generator=g) - 0.5) / 0.28209479177387814
    shs[:, 1:, :] = 0.1 * torch.randn(P, 15, 3, generator=g)
    cloud = dict(means3D=torch.stack([x, y, z], 1).float().contiguous(), scales=s.float().contiguous(),
                 rotations=(q / q.norm(dim=1, keepdim=True)).float().contiguous(),
                 opacities=torch.sigmoid(1.5 * torch.randn(P, 1, generator=g)).float().contiguous(), shs=shs.float().contiguous())
    return cam, cloud


@functools.lru_cache(maxsize=None)
def make(name, seed=None):
    """dict: cam, cloud (activated attributes), degree, g_color (3,H,W), scale_modifier, colors_precomp, cov3D_precomp, names
    (the gradient tensors the case produces)."""
    seed = SEEDS[name] if seed is None else seed
    case = dict(name=name, degree=3, scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None, names=NAMES_SH, g_seed=1)
    if name.startswith("sparse_deg"):
        cam, cloud = hp.box_setup(300, 64, 64, seed)
        case["degree"] = int(name[-1])
    elif name == "occluded":
        cam, cloud = hp.box_setup(300, 64, 64, seed, scale_mult=3.0)
    elif name == "posed":
        cam, cloud = pc.box_scene("general", 300, 77, 53, seed)
    elif name == "fov_clamp":
        cam = cameras.identity_camera(96, 64)
        rng = np.random.Generator(np.random.PCG64(seed))
        cloud = _t(ref_cases._cloud(rng, 300, (-6, -4, 1.0), (6, 4, 4.0), 0.5, sigma=0.4))
        case["degree"] = 1
    elif name == "sh_clamp":
        cam, cloud = hp.box_setup(300, 72, 56, seed)
        cloud["shs"][:, 0] -= 1.0
    elif name == "precomp":
        cam, cloud = hp.box_setup(300, 64, 64, seed)
        cov = torch_oracle.cov3d_from_scale_rot(cloud["scales"].double(), 1.0, cloud["rotations"].double()).float().contiguous()
        cols = torch.rand(300, 3, generator=torch.Generator().manual_seed(100 + seed))
        case.update(degree=0, colors_precomp=cols, cov3D_precomp=cov, names=NAMES_PRE)
    elif name == "scale_modifier":
        cam, cloud = hp.box_setup(300, 64, 48, seed)
        case.update(degree=2, scale_modifier=1.7)
    elif name == "long_lists":
        cam, cloud = hp.box_setup(400, 32, 32, seed, scale_mult=4.0)
        case["degree"] = 1
    elif name == "constant_upstream":
        cam, cloud = _on_screen_cloud(250, 96, 80, seed)
    else:
        raise ValueError(name)
    H, W = cam.image_height, cam.image_width
    g = torch.ones(3, H, W) if name == "constant_upstream" else synthetic.upstream_grad(H, W, case["g_seed"])
    case.update(cam=cam, cloud=cloud, g_color=g)
    return case


def upstream_depth(case):
    return torch.randn(1, case["cam"].image_height, case["cam"].image_width, generator=torch.Generator().manual_seed(3))


def upstream_alpha(case):
    return torch.randn(1, case["cam"].image_height, case["cam"].image_width, generator=torch.Generator().manual_seed(21))


def view_camera(case, view):
    """The case's own camera (view None) or camera `view` of the multi-view step on the case's image size."""
    cam = case["cam"]
    return cam if view is None else pc.camera(VIEW_POSES[view], cam.image_width, cam.image_height)


def view_upstream(case, view):
    return case["g_color"] if view is None else synthetic.upstream_grad(case["cam"].image_height, case["cam"].image_width, 30 + view)


# ---- the C oracle -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def c_oracle(name, seed=None, view=None):
    """helpers.run_oracle's dict (float32 gradients of <g_color, colour>, and the stage() with the fragile pixels)."""
    case = make(name, seed)
    return hp.run_oracle(case["cloud"], view_camera(case, view), case["degree"], torch.tensor(BG), view_upstream(case, view),
                         colors_precomp=case["colors_precomp"], cov3D_precomp=case["cov3D_precomp"],
                         scale_modifier=case["scale_modifier"])


# ---- autograd through the torch restatements -------------------------------------------------------------------------------
def aa_coef(means3D, cam, scales, rotations, scale_modifier, dtype):
    """tests/aa_ref.coef64 in `dtype`: aa_ref's own float64 chain is the reference; the float32 calibrator needs the same chain
    evaluated in float32, cancellation of det0 included."""
    if dtype == torch.float64:
        tfx, tfy = hp.tan_fov(cam)
        return aa_ref.coef64(means3D, cam.world_view_transform, tfx, tfy, cam.image_width, cam.image_height, scales, rotations,
                             scale_modifier)
    V = cam.world_view_transform.to(dtype)
    tfx, tfy = hp.tan_fov(cam)
    W, H = cam.image_width, cam.image_height
    fx, fy = W / (2.0 * tfx), H / (2.0 * tfy)
    cov3D = torch_oracle.cov3d_from_scale_rot(scales, scale_modifier, rotations)
    pv = means3D @ V[:3, :3] + V[3, :3]
    tz = pv[:, 2]
    tz_safe = torch.where(tz > 0.2, tz, torch.ones_like(tz))
    limx, limy = 1.3 * tfx, 1.3 * tfy
    txtz, tytz = pv[:, 0] / tz_safe, pv[:, 1] / tz_safe
    tx = torch.where((txtz < -limx) | (txtz > limx), (txtz.clamp(-limx, limx) * tz_safe).detach(), pv[:, 0])
    ty = torch.where((tytz < -limy) | (tytz > limy), (tytz.clamp(-limy, limy) * tz_safe).detach(), pv[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz_safe, zero, -(fx * tx) / (tz_safe * tz_safe),
                     zero, fy / tz_safe, -(fy * ty) / (tz_safe * tz_safe)], dim=1).reshape(-1, 2, 3)
    A = J @ V[:3, :3].T
    Sig = torch.stack([cov3D[:, 0], cov3D[:, 1], cov3D[:, 2], cov3D[:, 1], cov3D[:, 3], cov3D[:, 4],
                       cov3D[:, 2], cov3D[:, 4], cov3D[:, 5]], dim=1).reshape(-1, 3, 3)
    c2 = A @ Sig @ A.transpose(1, 2)
    a0, b, c0 = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
    a, c = a0 + aa_ref.H_DILATION, c0 + aa_ref.H_DILATION
    rho = (a0 * c0 - b * b) / (a * c - b * b)
    coef = torch.where(rho > aa_ref.RHO_FLOOR, torch.sqrt(rho.clamp_min(aa_ref.RHO_FLOOR)),
                       torch.full_like(rho, aa_ref.RHO_FLOOR ** 0.5))
    return torch.where(tz > 0.2, coef, torch.ones_like(coef))


def _leaves(case, dtype):
    d = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
    cloud = case["cloud"]
    pre_cov, pre_col = case["cov3D_precomp"] is not None, case["colors_precomp"] is not None
    # The reference's backward differentiates with respect to the MODIFIED scale mod * s (its computeCov3D forms dL/dscale from
    # s = mod * scale and never multiplies by mod; oracle/raster_oracle.c and the kernels keep that, tests/test_gpu_aa.py
    # _coef_grad_terms): the leaf is mod * s, and the restatements render it with a modifier of 1.
    lv = dict(means3D=d(cloud["means3D"]), opacity=d(cloud["opacities"]),
              scales=None if pre_cov else d(cloud["scales"].to(dtype) * case["scale_modifier"]),
              rotations=None if pre_cov else d(cloud["rotations"]),
              cov3D=d(case["cov3D_precomp"]), colors=d(case["colors_precomp"]), sh=None if pre_col else d(cloud["shs"]))
    lv["means2D"] = torch.zeros(cloud["means3D"].shape, dtype=dtype, requires_grad=True)
    return lv


def _render(case, lv, dtype, cam, mode, opacity=None, shs=None, scales=None, rotations=None, with_layers=False):
    """(colour, depth, alpha) of the leaves; mode "color": oracle/torch_oracle.render (depth without a gradient, alpha None),
    else tests/grad_oracle.render with differentiable depth and alpha."""
    tfx, tfy = hp.tan_fov(cam)
    pick = lambda over, k: lv[k] if over is None else over
    args = (lv["means3D"], pick(opacity, "opacity"), cam.world_view_transform, cam.full_proj_transform, cam.camera_center, tfx,
            tfy, cam.image_height, cam.image_width, torch.tensor(BG))
    kw = dict(scales=pick(scales, "scales"), rotations=pick(rotations, "rotations"), scale_modifier=1.0,
              cov3D_precomp=lv["cov3D"], shs=pick(shs, "sh"), degree=case["degree"], colors_precomp=lv["colors"],
              means2D=lv["means2D"], dtype=dtype)
    if mode == "color":
        col, dep, _ = torch_oracle.render(*args, **kw)
        return col, dep, None
    col, dep, alpha, _ = grad_oracle.render(*args, alpha=True, **kw)
    return col, dep, alpha


def _loss(case, col, dep, alpha, mode, g_color):
    dt = col.dtype
    terms = []
    if mode in ("color", "aa", "all"):
        terms.append((col * g_color.to(dt)).sum())
    if mode in ("depth", "all"):
        terms.append((dep * upstream_depth(case).to(dt)).sum())
    if mode in ("alpha", "all"):
        terms.append((alpha * upstream_alpha(case).to(dt)).sum())
    return sum(terms)


def _collect(lv, names):
    out = {}
    for k in names:
        g = lv[k].grad
        out[k] = (torch.zeros_like(lv[k]) if g is None else g).detach().double().numpy()
    return out


@functools.lru_cache(maxsize=None)
def torch_grads(name, dtype=torch.float64, mode="color", seed=None, view=None):
    """Gradients (float64 numpy arrays by helpers' names) of the mode's loss by autograd in `dtype`.
    mode: "color" <g_color, colour> through torch_oracle.render; "depth" / "alpha": <g, depth> / <g, alpha> alone and "all": the
    three together, through grad_oracle.render; "aa": colour, with the opacities times the anti-aliasing coefficient.
    view: a camera of VIEW_POSES with its own upstream gradient instead of the case's."""
    case = make(name, seed)
    cam = view_camera(case, view)
    lv = _leaves(case, dtype)
    op = None
    if mode == "aa":
        op = lv["opacity"] * aa_coef(lv["means3D"], cam, lv["scales"], lv["rotations"], 1.0, dtype)[:, None]
    col, dep, alpha = _render(case, lv, dtype, cam, "color" if mode == "aa" else mode, opacity=op)
    _loss(case, col, dep, alpha, mode, view_upstream(case, view)).backward()
    return _collect(lv, case["names"])


@functools.lru_cache(maxsize=None)
def view_sum(name, dtype=torch.float64):
    """The multi-view step's expectation: the sum over VIEW_POSES of every view's gradients, added in float64."""
    per = [torch_grads(name, dtype, "color", None, v) for v in range(len(VIEW_POSES))]
    return {k: sum(p[k] for p in per) for k in per[0]}


@functools.lru_cache(maxsize=None)
def view_sum_c(name):
    per = [c_oracle(name, None, v)["grads"] for v in range(len(VIEW_POSES))]
    return {k: sum(p[k].astype(np.float64) for p in per) for k in make(name)["names"]}


# ---- the raw path: stored parameters, activations written in torch in front of the oracle -----------------------------------
@functools.lru_cache(maxsize=None)
def raw_cloud(name):
    """(GaussianCloud on the CPU holding logit opacities, log scales, quaternions with norms from 0.5 to 2 and the SH split in
    two; the activated attributes as torch's float32 activations give them, for the C oracle's fragile pixels)."""
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    case = make(name)
    cloud = case["cloud"]
    g = torch.Generator().manual_seed(5)
    rot = cloud["rotations"] * (0.5 + 1.5 * torch.rand(cloud["rotations"].shape[0], 1, generator=g))
    stored = GaussianCloud(cloud["means3D"], cloud["scales"], rot, cloud["opacities"], cloud["shs"], active_sh_degree=case["degree"])
    with torch.no_grad():
        act = dict(means3D=stored._xyz.detach().clone(), shs=stored.get_features.contiguous(), opacities=stored.get_opacity,
                   scales=stored.get_scaling, rotations=stored.get_rotation)
    return stored, act


@functools.lru_cache(maxsize=None)
def raw_c_oracle(name):
    case = make(name)
    return hp.run_oracle(raw_cloud(name)[1], case["cam"], case["degree"], torch.tensor(BG), case["g_color"])


@functools.lru_cache(maxsize=None)
def raw_torch_grads(name, dtype=torch.float64):
    """Gradients with respect to the STORED parameters (RAW_NAMES): exp, normalize, sigmoid and the dc | rest concatenation in
    `dtype`, then torch_oracle.render."""
    case = make(name)
    stored, _ = raw_cloud(name)
    d = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    raw = {n: d(getattr(stored, n)) for n in RAW_NAMES[1:]}
    lv = dict(means3D=raw["_xyz"], cov3D=None, colors=None,
              means2D=torch.zeros(raw["_xyz"].shape, dtype=dtype, requires_grad=True))
    col, _, _ = _render(case, lv, dtype, case["cam"], "color", opacity=torch.sigmoid(raw["_opacity"]),
                        shs=torch.cat([raw["_features_dc"], raw["_features_rest"]], dim=1), scales=torch.exp(raw["_scaling"]),
                        rotations=torch.nn.functional.normalize(raw["_rotation"]))
    (col * case["g_color"].to(dtype)).sum().backward()
    raw["means2D"] = lv["means2D"]
    return _collect(raw, RAW_NAMES)


# ---- AbsGS: sum over the pixels of |that pixel's share of dL/dmeans2D| ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def abs_reference(name, dtype=torch.float64):
    """(abs, signed), (P, 2) float64 numpy each: what tests/absgrad_ref.reference computes (every pixel's share of dL/dmeans2D, the
    magnitudes summed) on a case of this file.  There one autograd.grad per pixel; here grad_oracle's pixel_probe gives every
    share from ONE backward.  The signed sum of the shares must be the whole-image dL/dmeans2D: tests/test_rowbar_cpu.py."""
    case = make(name)
    cam = case["cam"]
    lv = _leaves(case, dtype)
    tfx, tfy = hp.tan_fov(cam)
    probe = []
    col = grad_oracle.render(lv["means3D"], lv["opacity"], cam.world_view_transform, cam.full_proj_transform, cam.camera_center,
                             tfx, tfy, cam.image_height, cam.image_width, torch.tensor(BG), scales=lv["scales"],
                             rotations=lv["rotations"], shs=lv["sh"], degree=case["degree"], means2D=lv["means2D"], dtype=dtype,
                             pixel_probe=probe)[0]
    (col * case["g_color"].to(dtype)).sum().backward()
    P = lv["means2D"].shape[0]
    ndc = torch.tensor([0.5 * cam.image_width, 0.5 * cam.image_height], dtype=torch.float64)       # pixels per NDC unit
    abs_sum, signed = torch.zeros(P, 2, dtype=torch.float64), torch.zeros(P, 2, dtype=torch.float64)
    for ids, _, E in probe:
        g = E.grad.double() * ndc
        abs_sum.index_add_(0, ids, g.abs().sum(0))
        signed.index_add_(0, ids, g.sum(0))
    return abs_sum.numpy(), signed.numpy()


# ---- what a case is there for ----------------------------------------------------------------------------------------------
def list_lengths(name):
    """Entries per tile list [tiles_y, tiles_x], from the C oracle's means2D and radii (the rectangle rule of the binning)."""
    c = c_oracle(name)
    cam = make(name)["cam"]
    gx, gy = (cam.image_width + 15) // 16, (cam.image_height + 15) // 16
    m2, r = c["res"].stage()["means2D"], c["radii"]
    count = np.zeros((gy, gx), dtype=np.int64)
    for i in np.nonzero(r > 0)[0]:
        x0, x1 = np.clip([int((m2[i, 0] - r[i]) / 16), int((m2[i, 0] + r[i] + 15) / 16)], 0, gx)
        y0, y1 = np.clip([int((m2[i, 1] - r[i]) / 16), int((m2[i, 1] + r[i] + 15) / 16)], 0, gy)
        count[y0:y1, x0:x1] += 1
    return count


def clamp_classes(case):
    """(x only, y only): boolean masks of the Gaussians in front of the near plane beyond 1.3 tan(fov/2) in one direction only."""
    cam = case["cam"]
    V = cam.world_view_transform.double()
    pv = case["cloud"]["means3D"].double() @ V[:3, :3] + V[3, :3]
    tfx, tfy = hp.tan_fov(cam)
    front = pv[:, 2] > 0.2
    bx = front & ((pv[:, 0] / pv[:, 2]).abs() > 1.3 * tfx)
    by = front & ((pv[:, 1] / pv[:, 2]).abs() > 1.3 * tfy)
    return (bx & ~by).numpy(), (by & ~bx).numpy()
