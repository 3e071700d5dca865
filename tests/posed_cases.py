"""Posed cameras (test helper, not collected): the named poses, the two scenes and the seeded cases shared by
tests/test_posed_cases_cpu.py -- which checks on the CPU that every case is fit for its GPU comparison and sensitive to the
camera bugs it aims at -- and tests/test_gpu_posed.py.

A pose is a camera-to-world matrix in the convention cameras.make_camera expects (COLMAP axes: y down, z forward),
R = Ry(yaw) Rx(pitch) Rz(roll), then a translation.  Two scenes:
  box:  synthetic.make_cloud(P, "box", seed), made in the CAMERA frame and carried to the world by c2w in float64 (then rounded
        to float32): the camera sees the familiar load from any pose;
  band: synthetic.make_cloud(P, "band", seed) as it is, a ring around the world origin: Gaussians behind the camera, across the
        near plane and beyond the field-of-view clamp under a general view matrix.
References are computed once per process and case (functools.lru_cache); callers do not modify them."""
import functools
import math

import numpy as np
import torch

from luciddreamer_amd import cameras, synthetic
from tests import helpers as hp

NAMES_SH = ("means2D", "opacity", "means3D", "sh", "scales", "rotations")
NAMES_PRE = ("means2D", "colors", "opacity", "means3D", "cov3D")
BG = (0.1, 0.3, 0.7)

# name: (yaw, pitch, roll, translation)
POSES = {
    "translated": (0.0, 0.0, 0.0, (0.7, -0.4, -1.3)),          # campos, V[12..14], Pm[12..15] with a trivial rotation
    "pitched": (0.0, 0.35, 0.0, (0.0, 0.0, 0.0)),              # V[5], V[6], V[9]
    "rolled": (0.0, 0.0, 0.6, (0.0, 0.0, 0.0)),                # V[0], V[1], V[4], V[5]
    "general": (0.5, -0.3, 0.8, (1.1, -0.6, 0.9)),             # everything at once
    "llff": (0.02, -0.015, 0.0, (0.097, -0.098, 0.137)),       # the size of the llff presets: what a tolerance could hide
    "back": (0.0, 0.0, 0.0, (0.0, 0.0, -5.0)),                 # the extent of back.json: |campos| above the scene depth
}
# the four world poses of the band scene
BAND_POSES = [
    (0.7, 0.2, 0.3, (0.8, -0.3, 1.5)),
    (-2.0, -0.25, 0.0, (-1.2, 0.4, -0.9)),
    (3.0, 0.0, -0.5, (0.3, 0.6, 2.4)),
    (1.4, 0.0, 0.0, (2.5, 0.0, 0.0)),
]


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)


def c2w_of(pose):
    yaw, pitch, roll, t = pose
    m = np.eye(4)
    m[:3, :3] = rot_y(yaw) @ rot_x(pitch) @ rot_z(roll)
    m[:3, 3] = t
    return m


def camera(pose, W, H):
    """pose: a name of POSES, or a (yaw, pitch, roll, translation) tuple."""
    return cameras.make_camera(c2w_of(POSES[pose] if isinstance(pose, str) else pose), W, H)


def box_scene(pose, P, W, H, seed):
    cam = camera(pose, W, H)
    cloud = synthetic.make_cloud(P, "box", seed)
    m = c2w_of(POSES[pose])
    world = cloud["means3D"].double().numpy() @ m[:3, :3].T + m[:3, 3]
    cloud["means3D"] = torch.from_numpy(world.astype(np.float32)).contiguous()
    return cam, cloud


def band_scene(pose, W, H, seed, P=6000):
    return camera(pose, W, H), synthetic.make_cloud(P, "band", seed)


# ---- the operator cases ------------------------------------------------------------------------------------------------------
# name: (scene, pose, SH degree, P, W, H, seed).  97 x 61 and 131 x 77 are ragged in both directions, 192 x 112 and 160 x 96 are
# whole 16 x 16 tiles.  The seeds are the first ones at which the CPU oracle flags NO pixel as sitting on a discrete threshold
# (tests/test_posed_cases_cpu.py asserts it), so that the gradients are held to the whole-tensor bar.
OP_CASES = {
    "box_translated": ("box", "translated", 3, 1500, 97, 61, 7),
    "box_pitched": ("box", "pitched", 0, 3000, 192, 112, 1),
    "box_rolled": ("box", "rolled", 1, 1500, 97, 61, 7),
    "box_general": ("box", "general", 3, 1500, 97, 61, 2),
    "box_llff": ("box", "llff", 2, 3000, 192, 112, 3),
    "box_back": ("box", "back", 1, 1500, 97, 61, 7),
    "band_0": ("band", 0, 2, 6000, 160, 96, 6),
    "band_1": ("band", 1, 3, 6000, 131, 77, 3),
    "band_2": ("band", 2, 0, 6000, 160, 96, 7),
    "band_3": ("band", 3, 1, 6000, 131, 77, 6),
}
PRECOMP_CASE = "box_general"         # colours and 3D covariances given by the caller: no SH, so campos is unused
RAW_CASES = ("box_general", "box_translated")
MODE_CASES = ("box_pitched", "box_translated", "box_general")        # depth and alpha outputs, float64 reference
AA_CASE = "box_general"
AA_SEED = 0                          # its own seed: the cloud gains the special Gaussians of tests/aa_cases.py

# ---- the multi-view step: five different poses in one call, not in sorted order ---------------------------------------------
STEP_POSES = ("general", "back", "pitched", "llff", "translated")
STEP_SCENE = (6000, 131, 77, 4)       # P, W, H, seed of the band cloud they all look at


def pose_of(case):
    scene, pose = OP_CASES[case][:2]
    return POSES[pose] if scene == "box" else BAND_POSES[pose]


@functools.lru_cache(maxsize=None)
def make(case):
    """(cam, cloud, degree) of an operator case."""
    scene, pose, degree, P, W, H, seed = OP_CASES[case]
    if scene == "box":
        cam, cloud = box_scene(pose, P, W, H, seed)
    else:
        cam, cloud = band_scene(BAND_POSES[pose], W, H, seed, P)
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
    """The stored parameters of an operator case (log-scales, logit-opacities, quaternions of any norm, SH split in two) as a
    CPU GaussianCloud, and the activated attributes the oracle is fed: torch's own float32 activations of them."""
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    cam, cloud, degree = make(case)
    g = torch.Generator().manual_seed(5)
    rot = cloud["rotations"] * (0.5 + 1.5 * torch.rand(cloud["rotations"].shape[0], 1, generator=g))
    pc = GaussianCloud(cloud["means3D"], cloud["scales"], rot, cloud["opacities"], cloud["shs"], active_sh_degree=degree)
    with torch.no_grad():
        act = dict(means3D=pc._xyz.detach().clone(), shs=pc.get_features.contiguous(), opacities=pc.get_opacity,
                   scales=pc.get_scaling, rotations=pc.get_rotation)
    return cam, pc, act, degree


@functools.lru_cache(maxsize=None)
def raw_reference(case):
    cam, _, act, degree = raw_cloud(case)
    return hp.run_oracle(act, cam, degree, torch.tensor(BG), upstream(cam, 4))


@functools.lru_cache(maxsize=None)
def step_scene():
    """(cams, cloud) of the multi-view step."""
    P, W, H, seed = STEP_SCENE
    return [camera(p, W, H) for p in STEP_POSES], synthetic.make_cloud(P, "band", seed)


def step_upstream(i):
    """View i's own dL/dcolor."""
    _, W, H, _ = STEP_SCENE
    return synthetic.upstream_grad(H, W, seed=30 + i)


@functools.lru_cache(maxsize=None)
def step_reference(i):
    cams, cloud = step_scene()
    return hp.run_oracle(cloud, cams[i], 3, torch.tensor(BG), step_upstream(i))


@functools.lru_cache(maxsize=None)
def aa_inputs():
    """(cam, cloud with the sub-pixel and the clamped Gaussians of tests/aa_cases.py placed in the camera's frame)."""
    from tests import aa_cases
    scene, pose, _, P, W, H, _ = OP_CASES[AA_CASE]
    seed = AA_SEED
    assert scene == "box"
    cam = camera(pose, W, H)
    cloud = aa_cases.with_special_gaussians(cameras.identity_camera(W, H), synthetic.make_cloud(P, "box", seed), seed)
    # without the needles: they are fit for float32 only while they lie along a screen axis of an unturned camera (there the 3D
    # covariance is diagonal); turned, det0 = a0 c0 - b b cancels and coef32 leaves coef64 by 5e-4 whatever the kernel does
    n = aa_cases.N_SPECIAL
    keep = torch.cat([torch.arange(0, P + n), torch.arange(P + 2 * n, P + 3 * n)])
    cloud = {k: v[keep].contiguous() for k, v in cloud.items()}
    m = c2w_of(POSES[pose])
    world = cloud["means3D"].double().numpy() @ m[:3, :3].T + m[:3, 3]
    cloud["means3D"] = torch.from_numpy(world.astype(np.float32)).contiguous()
    return cam, cloud


@functools.lru_cache(maxsize=None)
def aa_reference():
    """The anti-aliased render is the plain render of opacity * coef32 (tests/aa_ref.py): (oracle result on them, coef32)."""
    from tests import aa_cases
    cam, cloud = aa_inputs()
    coef = aa_cases.coef_of(cam, cloud)
    return hp.run_oracle(aa_cases.prescaled(cloud, coef), cam, 3, torch.tensor(BG), upstream(cam))


# ---- the camera, altered on the reference side --------------------------------------------------------------------------------
def altered(cam, how):
    """The camera a wrong kernel would in effect use.  "campos": the position at the origin; "translation": the view matrix's
    translation (V[12..14], row 3 of the row-vector storage) zeroed; "transposed": its 3 x 3 block transposed."""
    if how == "campos":
        return cam._replace(camera_center=torch.zeros(3))
    view = cam.world_view_transform.clone()
    if how == "translation":
        view[3, :3] = 0.0
    elif how == "transposed":
        view[:3, :3] = view[:3, :3].T.clone()
    else:
        raise ValueError(how)
    return cam._replace(world_view_transform=view.contiguous())


def aims(case):
    """The alterations a case is meant to catch, from its pose alone: campos where the camera is off the origin and the colour
    depends on the view direction (SH degree >= 1), the translation where there is one, the transposition where the camera
    is turned."""
    yaw, pitch, roll, t = pose_of(case)
    degree = OP_CASES[case][2]
    out = []
    if any(t) and degree >= 1:
        out.append("campos")
    if any(t):
        out.append("translation")
    if yaw or pitch or roll:
        out.append("transposed")
    return out
