"""Camera intrinsics (test helper, not collected): the named intrinsics, the scenes and the seeded cases shared by
tests/test_intrinsics_cases_cpu.py -- which checks on the CPU that every case is fit for its GPU comparison and sensitive to the
intrinsics bugs it aims at -- and tests/test_gpu_intrinsics.py.

Everywhere else in the suite a camera comes from cameras.make_camera: one field of view, FoVy from the aspect ratio (square
pixels, focal_x == focal_y), a centred principal point, znear = 0.01 and zfar = 100.  camera() here is
cameras.projection_matrix generalised to left != -right with the two tangents given independently; the view matrix and the
centre are make_camera's.  Every reference in tests/ reads only the MiniCam's fields, so these cameras plug in unchanged.

The scene is the box cloud of synthetic.make_cloud, made in the CAMERA frame, stretched to fill this frustum as it fills the
default one, then carried to the world by c2w in float64 (as posed_cases.box_scene does).
References are computed once per process and case (functools.lru_cache); callers do not modify them."""
import functools
import math

import numpy as np
import torch

from luciddreamer_amd import cameras, synthetic
from tests import helpers as hp
from tests import posed_cases as pc

NAMES_SH = pc.NAMES_SH
NAMES_PRE = pc.NAMES_PRE
BG = pc.BG
TAN_X_DEFAULT = math.tan(0.5 * cameras.FOVX_DEFAULT)
P_BOX = 1500


def camera(pose, W, H, tan_x, tan_y, shift=(0.0, 0.0), znear=0.01, zfar=100.0):
    """pose: a name of posed_cases.POSES, or a (yaw, pitch, roll, translation) tuple.  full_proj_transform = view @ P^T with
    P[0,0] = 1 / tan_x, P[1,1] = 1 / tan_y, P[0,2], P[1,2] = shift (the principal point's offset in NDC), P[3,2] = 1 and the
    third row from znear and zfar."""
    base = cameras.make_camera(pc.c2w_of(pc.POSES[pose] if isinstance(pose, str) else pose), W, H)
    view = base.world_view_transform
    full = (view @ projection(tan_x, tan_y, shift, znear, zfar).T.contiguous()).contiguous()
    return cameras.MiniCam(W, H, 2.0 * math.atan(tan_y), 2.0 * math.atan(tan_x), znear, zfar, view, full, base.camera_center)


def projection(tan_x, tan_y, shift, znear, zfar):
    P = torch.zeros(4, 4)
    P[0, 0] = 1.0 / tan_x
    P[1, 1] = 1.0 / tan_y
    P[0, 2] = shift[0]
    P[1, 2] = shift[1]
    P[3, 2] = 1.0
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = -(zfar * znear) / (zfar - znear)
    return P


def square(tan_x, W, H):
    """tan_y of square pixels."""
    return tan_x * H / W


# name: (W, H, tan_x, tan_y (None: square pixels), shift, pose, znear, zfar, SH degree, seed).  Every size but 160 x 96 and
# 96 x 112 is ragged in both directions; 96 x 112 is whole tiles.  The seeds are the first ones (from 0) at which the CPU oracle flags
# NO pixel of any reference the GPU tests take from the case -- its own, and the raw and own-colour ones where it has them -- and
# tests/test_intrinsics_cases_cpu.py passes; likewise AA_SEED and the step's seed.
INTRINSICS = {
    "wide": (97, 61, 1.5574, None, (0.0, 0.0), "translated", 0.01, 100.0, 3, 0),          # clamp limits, the cull constant g
    "narrow": (160, 96, 0.0756, None, (0.0, 0.0), "pitched", 0.01, 100.0, 0, 1),          # focal ~ 1060 px
    "tall_pixels": (131, 77, 0.45, 0.70, (0.0, 0.0), "rolled", 0.01, 100.0, 1, 0),        # focal_x ~ 2.6 focal_y
    "wide_pixels": (96, 112, 0.70, 0.30, (0.0, 0.0), "translated", 0.01, 100.0, 2, 0),    # focal_y > focal_x
    "off_centre": (97, 61, 0.4397, None, (0.35, -0.2), "translated", 0.01, 100.0, 1, 0),  # Pm[8], Pm[9]; the clamp on screen
    "general": (131, 77, 0.62, 0.27, (-0.3, 0.25), "general", 0.5, 20.0, 3, 0),           # everything at once
}
CASES = tuple(INTRINSICS)
PRECOMP_CASE = "general"
RAW_CASES = ("tall_pixels", "general")
MODE_CASES = ("tall_pixels", "off_centre", "general")
AA_CASE = "general"
AA_SEED = 1
SIDE_CASE = "general"                        # absolute gradient, median depth, normals, distortion, features
CULL_CASES = ("wide", "narrow", "off_centre")
CLAMP_CASES = ("wide", "off_centre", "general")

# ---- the multi-view step: five poses, five intrinsics in one call, not in sorted order ---------------------------------------
STEP_VIEWS = (("general", "general"), ("back", "wide"), ("pitched", "tall_pixels"), ("llff", "off_centre"),
              ("translated", "wide_pixels"))          # (pose, intrinsics row)
STEP_SCENE = (6000, 131, 77, 1)                       # P, W, H, seed of the band cloud they all look at


def tangents(name, W=None, H=None):
    """(tan_x, tan_y) of a row; W, H: re-derived for another image size where the row's pixels are square."""
    w, h, tx, ty = INTRINSICS[name][:4]
    W, H = (w, h) if W is None else (W, H)
    return tx, (square(tx, W, H) if ty is None else ty)


def row_camera(name, pose=None, W=None, H=None, znear=None, zfar=None):
    w, h, _, _, shift, p, zn, zf = INTRINSICS[name][:8]
    W, H = (w, h) if W is None else (W, H)
    tx, ty = tangents(name, W, H)
    return camera(p if pose is None else pose, W, H, tx, ty, shift, zn if znear is None else znear, zf if zfar is None else zfar)


def fit_to_frustum(cloud, name):
    """The camera-frame box cloud stretched to this row's frustum: x by tan_x / tan_x(default), y likewise, moved by
    -shift tan z, the scales by the geometric mean of the two ratios.  float64, rounded once."""
    W, H, _, _, shift = INTRINSICS[name][:5]
    tx, ty = tangents(name)
    rx, ry = tx / TAN_X_DEFAULT, ty / square(TAN_X_DEFAULT, W, H)
    m = cloud["means3D"].double().clone()
    m[:, 0] = m[:, 0] * rx - shift[0] * tx * m[:, 2]
    m[:, 1] = m[:, 1] * ry - shift[1] * ty * m[:, 2]
    out = dict(cloud)
    out["means3D"] = m
    out["scales"] = (cloud["scales"].double() * math.sqrt(rx * ry)).float().contiguous()
    return out


def to_world(cloud, pose):
    m = pc.c2w_of(pc.POSES[pose] if isinstance(pose, str) else pose)
    world = cloud["means3D"].double().numpy() @ m[:3, :3].T + m[:3, 3]
    out = dict(cloud)
    out["means3D"] = torch.from_numpy(world.astype(np.float32)).contiguous()
    return out


def box_scene(name, seed, P=P_BOX):
    pose = INTRINSICS[name][5]
    return row_camera(name), to_world(fit_to_frustum(synthetic.make_cloud(P, "box", seed), name), pose)


@functools.lru_cache(maxsize=None)
def make(case):
    """(cam, cloud, degree) of an operator case."""
    degree, seed = INTRINSICS[case][8:10]
    cam, cloud = box_scene(case, seed)
    return cam, cloud, degree


def upstream(cam, seed=1):
    return synthetic.upstream_grad(cam.image_height, cam.image_width, seed)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The C oracle's forward and backward of an operator case (helpers.run_oracle's dict), background BG."""
    cam, cloud, degree = make(case)
    return hp.run_oracle(cloud, cam, degree, torch.tensor(BG), upstream(cam))


@functools.lru_cache(maxsize=None)
def precomp_inputs():
    from oracle import torch_oracle
    cam, cloud, _ = make(PRECOMP_CASE)
    P = cloud["means3D"].shape[0]
    cov = torch_oracle.cov3d_from_scale_rot(cloud["scales"].double(), 1.0, cloud["rotations"].double()).float()
    cols = torch.rand(P, 3, generator=torch.Generator().manual_seed(5))
    return cam, cloud, cols, cov


@functools.lru_cache(maxsize=None)
def precomp_reference():
    cam, cloud, cols, cov = precomp_inputs()
    return hp.run_oracle(cloud, cam, 0, torch.tensor(BG), upstream(cam), colors_precomp=cols, cov3D_precomp=cov)


def raw_cloud(case):
    """As posed_cases.raw_cloud: the stored parameters of an operator case as a CPU GaussianCloud, and the activated attributes
    the oracle is fed."""
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    cam, cloud, degree = make(case)
    g = torch.Generator().manual_seed(5)
    rot = cloud["rotations"] * (0.5 + 1.5 * torch.rand(cloud["rotations"].shape[0], 1, generator=g))
    model = GaussianCloud(cloud["means3D"], cloud["scales"], rot, cloud["opacities"], cloud["shs"], active_sh_degree=degree)
    with torch.no_grad():
        act = dict(means3D=model._xyz.detach().clone(), shs=model.get_features.contiguous(), opacities=model.get_opacity,
                   scales=model.get_scaling, rotations=model.get_rotation)
    return cam, model, act, degree


@functools.lru_cache(maxsize=None)
def raw_reference(case):
    cam, _, act, degree = raw_cloud(case)
    return hp.run_oracle(act, cam, degree, torch.tensor(BG), upstream(cam, 4))


@functools.lru_cache(maxsize=None)
def aa_inputs():
    """(cam, cloud): the case's cloud with the sub-pixel and the clamped Gaussians of tests/aa_cases.py placed in the camera's
    frame -- without the needles, for the reason posed_cases.aa_inputs gives."""
    from tests import aa_cases
    pose = INTRINSICS[AA_CASE][5]
    seed = AA_SEED
    cam = row_camera(AA_CASE)
    base = fit_to_frustum(synthetic.make_cloud(P_BOX, "box", seed), AA_CASE)
    base["means3D"] = base["means3D"].float()
    cloud = aa_cases.with_special_gaussians(row_camera(AA_CASE, pose=(0.0, 0.0, 0.0, (0.0, 0.0, 0.0))), base, seed)
    n = aa_cases.N_SPECIAL
    keep = torch.cat([torch.arange(0, P_BOX + n), torch.arange(P_BOX + 2 * n, P_BOX + 3 * n)])
    cloud = {k: v[keep].contiguous() for k, v in cloud.items()}
    return cam, to_world(cloud, pose)


@functools.lru_cache(maxsize=None)
def aa_reference():
    """The anti-aliased render is the plain render of opacity * coef32 (tests/aa_ref.py): the oracle's result on them."""
    from tests import aa_cases
    cam, cloud = aa_inputs()
    coef = aa_cases.coef_of(cam, cloud)
    return hp.run_oracle(aa_cases.prescaled(cloud, coef), cam, 3, torch.tensor(BG), upstream(cam))


@functools.lru_cache(maxsize=None)
def step_scene():
    """(cams, cloud) of the multi-view step."""
    P, W, H, seed = STEP_SCENE
    return [row_camera(row, pose=pose, W=W, H=H) for pose, row in STEP_VIEWS], synthetic.make_cloud(P, "band", seed)


def step_upstream(i):
    """View i's own dL/dcolor."""
    _, W, H, _ = STEP_SCENE
    return synthetic.upstream_grad(H, W, seed=30 + i)


@functools.lru_cache(maxsize=None)
def step_reference(i):
    cams, cloud = step_scene()
    return hp.run_oracle(cloud, cams[i], 3, torch.tensor(BG), step_upstream(i))


# ---- the camera, altered on the reference side --------------------------------------------------------------------------------
def altered(cam, how):
    """The camera a wrong kernel would in effect use.  "square": FoVy from FoVx and the aspect ratio (focal_y := focal_x);
    "swapped": FoVx and FoVy exchanged; "centred": the projection rebuilt without the principal point's shift; "first_view":
    the tangents of the step's view 0.  The first, second and last leave the matrices alone, as the kernels take the tangents
    and the projection matrix independently."""
    if how == "square":
        return cam._replace(FoVy=cameras.fovy_from_fovx(cam.FoVx, cam.image_width, cam.image_height))
    if how == "swapped":
        return cam._replace(FoVx=cam.FoVy, FoVy=cam.FoVx)
    if how == "first_view":
        first = step_scene()[0][0]
        return cam._replace(FoVx=first.FoVx, FoVy=first.FoVy)
    if how == "centred":
        P = projection(math.tan(0.5 * cam.FoVx), math.tan(0.5 * cam.FoVy), (0.0, 0.0), cam.znear, cam.zfar)
        return cam._replace(full_proj_transform=(cam.world_view_transform @ P.T.contiguous()).contiguous())
    raise ValueError(how)


def aims(case):
    """The alterations a case is meant to catch, from its row alone."""
    W, H, tx, ty, shift = INTRINSICS[case][:5]
    out = []
    if ty is not None:
        out += ["square", "swapped"]
    if any(shift):
        out.append("centred")
    return out


# ---- the side outputs on SIDE_CASE: the references of their own suites, which take the camera as an argument ------------------
# Each forward bar is that suite's: 4 x the distance of the float32 walk from the float64 render on the non-fragile pixels, taken
# here per run on the CPU (the suites record it per named input: render_normals_ref.FWD_ERR and its siblings).  The upstreams are
# zero on the pixels a walk flags; the gradients are float64 autograd's.
SIDE_MAPPING = "linear"
SIDE_CHANNELS = 19                           # feature_ref.K + 3: a full chunk and a tail


def _frozen(out):
    for v in out.values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def side_stage():
    cam, cloud, degree = make(SIDE_CASE)
    ref = hp.run_oracle(cloud, cam, degree, torch.tensor(BG))
    return ref, ref["res"].stage()


@functools.lru_cache(maxsize=None)
def median_reference():
    """dict(ids, depth, fragile, st): median_ref.walk on the oracle's stage."""
    from tests import median_ref as mr
    cam = make(SIDE_CASE)[0]
    _, st = side_stage()
    ids, depth, fragile = mr.walk(st, cam.image_width, cam.image_height)
    return dict(ids=ids, depth=depth, fragile=fragile, st=st)


@functools.lru_cache(maxsize=None)
def normals_reference():
    """dict(N64, layers64, fragile, G, leaf, margin, visible, fwd_err), as render_normals_ref.reference."""
    from tests import render_normals_ref as rn
    cam, cloud, degree = make(SIDE_CASE)
    H, W = cam.image_height, cam.image_width
    ref, st = side_stage()
    gn32 = rn.gauss_normals32(cloud["means3D"].numpy(), cloud["scales"].numpy(), cloud["rotations"].numpy(),
                              cam.world_view_transform.numpy(), ref["radii"])
    N32, _, fragile = rn.walk32(st, W, H, gn32)
    G = rn.upstream(H, W, fragile)
    leaf, _, N64, layers64, inter = rn.grads64(cloud, cam, degree, torch.tensor(BG), G.numpy())
    N64, layers64 = np.asarray(N64), np.asarray(layers64)
    return _frozen(dict(N64=N64, layers64=layers64, fragile=fragile, G=G, leaf=leaf, margin=inter["margin"].numpy(),
                        visible=np.asarray(ref["radii"]) > 0,
                        fwd_err=float(np.abs(N32.astype(np.float64) - N64)[:, ~fragile].max())))


@functools.lru_cache(maxsize=None)
def distortion_reference():
    """dict(D64, layers64, fragile, G, leaf, fwd_err), as distort_ref.reference(name, SIDE_MAPPING)."""
    from tests import distort_ref as dr
    cam, cloud, degree = make(SIDE_CASE)
    H, W = cam.image_height, cam.image_width
    coef = dr.coefficients(SIDE_MAPPING)
    _, st = side_stage()
    D32, _, fragile, _ = dr.walk32(st, W, H, coef)
    G = dr.upstream(H, W, fragile)
    leaf, _, D64, layers64 = dr.grads64(cloud, cam, degree, torch.tensor(BG), coef, G.numpy())
    D64, layers64 = np.asarray(D64).reshape(H, W), np.asarray(layers64)
    return _frozen(dict(D64=D64, layers64=layers64, fragile=fragile, G=G, leaf=leaf,
                        fwd_err=float(np.abs(D32.astype(np.float64) - D64)[~fragile].max())))


@functools.lru_cache(maxsize=None)
def features_reference():
    """dict(feats, F64, layers32, fragile, G, leaf, visible, fwd_err), as feature_ref.reference at SIDE_CHANNELS channels."""
    from tests import feature_ref as fr
    cam, cloud, _ = make(SIDE_CASE)
    H, W, C = cam.image_height, cam.image_width, SIDE_CHANNELS
    ref, st = side_stage()
    feats = (2.0 * torch.rand(cloud["means3D"].shape[0], C, generator=torch.Generator().manual_seed(53)) - 1.0).float().contiguous()
    F32, layers32, fragile = fr.walk32(st, W, H, feats.numpy())
    G = fr.upstream(C, H, W, fragile)
    leaf, F64 = fr.grads64(cloud, cam, feats, G.numpy())
    return _frozen(dict(feats=feats, F64=F64, layers32=layers32, fragile=fragile, G=G, leaf=leaf, visible=np.asarray(ref["radii"]) > 0,
                        fwd_err=float(np.abs(F32.astype(np.float64) - F64)[:, ~fragile].max())))
