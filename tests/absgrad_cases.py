"""Seeded inputs of the absgrad (AbsGS) tests (test helper, not collected), shared by tests/test_absgrad_cpu.py -- which checks
on the CPU that they are fit for the GPU comparisons -- and tests/test_gpu_absgrad.py.  The smallest shapes at which the
kernels can go wrong: partial tiles, Gaussians that own several instance slots, a list longer than two staging rounds of the
2-wave blend backward with pixels that stop early.

A case is a dict: cam, cloud (activated attributes, SH degree 1), bg, g_color (3,H,W), g_depth / g_alpha ((1,H,W) or None),
strict, antialiasing."""
import math

import torch

from luciddreamer_amd import cameras

DEGREE, SH_COEFFS = 1, 4
BATCH2 = 64                 # staged Gaussians per round of the 2-wave blend backward (csrc/render_bwd.hip)
NAMES = ("partial", "cancel", "long", "partial_depth_alpha", "partial_strict", "partial_aa")
# the committed seeds: tests/test_absgrad_cpu.py checks that the oracle alone leaves every one of them inside the GPU test's
# cap on left-out rows (rows of Gaussians that touch a threshold-fragile pixel: at most 1 in 50 of the visible rows)
SEEDS = {"partial": 11, "long": 5}
FRAGILE_ROW_CAP = 1.0 / 50.0


def tan_fov(cam):
    return math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)


def _pack(means, scales, opac, g, colour=None):
    P = means.shape[0]
    q = torch.randn(P, 4, generator=g)
    shs = torch.zeros(P, SH_COEFFS, 3)
    if colour is None:
        shs[:, 0, :] = (torch.rand(P, 3, generator=g) - 0.5) / 0.28209479177387814
        shs[:, 1:, :] = 0.1 * torch.randn(P, SH_COEFFS - 1, 3, generator=g)
    else:
        shs[:, 0, :] = (torch.tensor(colour) - 0.5) / 0.28209479177387814
    return dict(means3D=means.float().contiguous(), scales=scales.float().contiguous(),
                rotations=(q / q.norm(dim=1, keepdim=True)).float().contiguous(), opacities=opac.float().contiguous(),
                shs=shs.float().contiguous())


def _partial_cloud(cam, seed):
    """P = 64 in front of a 40 x 24 view (3 x 2 tiles, partial in both directions): 44 splats of 1.5 - 4 px, 8 broad ones (8 - 12 px:
    every one reaches four or more tiles, so k_gauss_bwd sums several instance slots), 6 behind the camera, 6 off screen."""
    g = torch.Generator().manual_seed(seed)
    tfx, tfy = tan_fov(cam)
    px = 2.0 * tfx / cam.image_width                     # world size of a pixel at unit depth

    def place(k, spread):
        z = 2.0 + 3.0 * torch.rand(k, generator=g)
        x = (torch.rand(k, generator=g) * 2 - 1) * spread * tfx * z
        y = (torch.rand(k, generator=g) * 2 - 1) * spread * tfy * z
        return torch.stack([x, y, z], 1), z

    m0, z0 = place(44, 0.9)
    s0 = (1.5 + 2.5 * torch.rand(44, 1, generator=g)) * px * z0[:, None] * torch.exp(0.3 * torch.randn(44, 3, generator=g))
    m1, z1 = place(8, 0.4)
    s1 = (8.0 + 4.0 * torch.rand(8, 1, generator=g)) * px * z1[:, None] * torch.exp(0.1 * torch.randn(8, 3, generator=g))
    m2, _ = place(6, 0.9)
    m2[:, 2] = -m2[:, 2]                                 # behind the camera
    s2 = 0.1 * torch.ones(6, 3)
    m3, z3 = place(6, 0.5)
    m3[:, 0] = torch.where(torch.rand(6, generator=g) < 0.5, -1.0, 1.0) * (2.0 + torch.rand(6, generator=g)) * tfx * z3   # off screen
    s3 = 2.0 * px * z3[:, None] * torch.ones(6, 3)
    means, scales = torch.cat([m0, m1, m2, m3]), torch.cat([s0, s1, s2, s3])
    opac = torch.sigmoid(1.5 * torch.randn(64, 1, generator=g)).clamp(0.05, 0.97)
    perm = torch.randperm(64, generator=g)               # the kinds interleaved in index order
    return _pack(means[perm], scales[perm], opac[perm], g)


def _cancel_cloud(cam):
    """One broad isotropic Gaussian (sigma 6 px, opacity 0.6, constant colour) centred on the four-tile corner of a 32 x 32 view."""
    tfx, _ = tan_fov(cam)
    z = 3.0
    sigma = 6.0 * (2.0 * tfx / cam.image_width) * z
    g = torch.Generator().manual_seed(0)
    cloud = _pack(torch.tensor([[0.0, 0.0, z]]), sigma * torch.ones(1, 3), torch.tensor([[0.6]]), g, colour=(0.8, 0.5, 0.3))
    cloud["rotations"] = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    return cloud


def _long_cloud(cam, seed):
    """P = 160 opaque, overlapping splats (3 - 5 px, opacity 0.7 - 0.95) centred inside tile (0, 0) of a 32 x 32 view: that tile's
    list is longer than two staging rounds (2 * BATCH2), and most of its pixels stop at T < 1e-4 after a few layers."""
    g = torch.Generator().manual_seed(seed)
    tfx, tfy = tan_fov(cam)
    W, H = cam.image_width, cam.image_height
    px = 2.0 * tfx / W
    P = 160
    z = 2.0 + 3.0 * torch.rand(P, generator=g)
    cx = 2.0 + 11.0 * torch.rand(P, generator=g)         # pixel coordinates of the centres
    cy = 2.0 + 11.0 * torch.rand(P, generator=g)
    x = ((2.0 * cx + 1.0) / W - 1.0) * tfx * z
    y = ((2.0 * cy + 1.0) / H - 1.0) * tfy * z
    s = (3.0 + 2.0 * torch.rand(P, 1, generator=g)) * px * z[:, None] * torch.exp(0.2 * torch.randn(P, 3, generator=g))
    opac = 0.7 + 0.25 * torch.rand(P, 1, generator=g)
    return _pack(torch.stack([x, y, z], 1), s, opac, g)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def make(name):
    assert name in NAMES, name
    case = dict(name=name, bg=torch.tensor([0.1, 0.2, 0.3]), g_depth=None, g_alpha=None, strict=False, antialiasing=False)
    if name.startswith("partial"):
        W, H = 40, 24
        cam = cameras.identity_camera(W, H)
        case.update(cam=cam, cloud=_partial_cloud(cam, SEEDS["partial"]), g_color=_randn(1, 3, H, W))
        if name == "partial_depth_alpha":
            case.update(g_depth=0.5 * _randn(2, 1, H, W), g_alpha=_randn(3, 1, H, W))
        case["strict"] = name == "partial_strict"
        case["antialiasing"] = name == "partial_aa"
    elif name == "cancel":
        cam = cameras.identity_camera(32, 32)
        # constant dL/dpixel, small enough that the float32 rounding of the cancelling signed sum stays far below the densification
        # threshold (0.0002) while the absolute sum stays far above it
        case.update(cam=cam, cloud=_cancel_cloud(cam), g_color=torch.full((3, 32, 32), 1e-3), bg=torch.zeros(3))
    else:
        cam = cameras.identity_camera(32, 32)
        case.update(cam=cam, cloud=_long_cloud(cam, SEEDS["long"]), g_color=_randn(4, 3, 32, 32))
    return case


def reference_cloud(case):
    """The cloud the float64 reference and the CPU oracle render: with anti-aliasing the opacities times the coefficient, which
    is what an anti-aliased render is by construction (tests/aa_ref.py); means2D does not enter the coefficient."""
    if not case["antialiasing"]:
        return case["cloud"]
    from tests import aa_cases
    return aa_cases.prescaled(case["cloud"], aa_cases.coef_of(case["cam"], case["cloud"]))
