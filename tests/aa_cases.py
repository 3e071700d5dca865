"""Seeded inputs of the anti-aliasing tests (test helper, not collected), shared by tests/test_aa_cpu.py -- which checks on the
CPU that they are fit for the GPU comparisons -- and tests/test_gpu_aa.py.

`python -m tests.aa_cases OUT.npz` renders the "off is off" view in a process that never touches the anti-aliasing setting."""
import math
import sys

import numpy as np
import torch

from luciddreamer_amd import cameras, synthetic
from tests import aa_ref

# (P, W, H, seed, scale_mult): box clouds in front of the identity camera.  scale_mult 0.3: most splats below a pixel.
FORWARD_CASES = [(6_000, 160, 128, 0, 1.0), (5_000, 256, 160, 3, 0.3)]
GRAD_CASES = [(5_000, 160, 128, 7, 1.0), (4_000, 192, 128, 9, 0.3)]
N_SPECIAL = 48            # per kind, appended to a gradient cloud: sub-pixel, needles, clamped (rho <= floor)


def tan_fov(cam):
    return math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)


def box_case(P, W, H, seed, scale_mult):
    cam = cameras.identity_camera(W, H)
    return cam, synthetic.make_cloud(P, "box", seed, scale_mult=scale_mult)


def with_special_gaussians(cam, cloud, seed, outside_clamp=False):
    """The cloud plus N_SPECIAL each of: sub-pixel blobs, needles (one long axis, two far below a pixel) and Gaussians so small
    that rho <= 0.000025 (the clamped branch: opacity near one, or they would not reach alpha = 1/255 at all), all placed in
    view; outside_clamp (the float64-only CPU checks) adds N_SPECIAL large ones beyond the 1.3 tan_fov clamp (off screen) and
    turns the needles at random."""
    g = torch.Generator().manual_seed(1000 + seed)
    tfx, tfy = tan_fov(cam)
    W = cam.image_width
    px = 2.0 * tfx / W                                   # world size of a pixel at unit depth
    n = N_SPECIAL

    def place(k, spread=0.8):
        z = 2.5 + 3.0 * torch.rand(k, generator=g)
        x = (torch.rand(k, generator=g) * 2 - 1) * spread * tfx * z
        y = (torch.rand(k, generator=g) * 2 - 1) * spread * tfy * z
        return torch.stack([x, y, z], 1), z

    parts = []
    m, z = place(n)                                      # sub-pixel: sigma 0.1 .. 0.5 px
    s = (0.1 + 0.4 * torch.rand(n, 1, generator=g)) * px * z[:, None] * torch.exp(0.2 * torch.randn(n, 3, generator=g))
    parts.append((m, s, torch.sigmoid(2.0 * torch.randn(n, 1, generator=g))))
    m, z = place(n)                                      # needles: 3 px long, 0.02 px thin
    s = torch.stack([3.0 * px * z, 0.02 * px * z, 0.02 * px * z], 1)
    parts.append((m, s, torch.sigmoid(2.0 * torch.randn(n, 1, generator=g))))
    m, z = place(n)                                      # clamped: sigma 0.02 px -> rho ~ 1.8e-6
    s = (0.02 * px * z)[:, None] * torch.ones(n, 3)
    parts.append((m, s, 0.9 + 0.09 * torch.rand(n, 1, generator=g)))
    if outside_clamp:
        z = 2.5 + 3.0 * torch.rand(n, generator=g)
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        x = sign * (1.35 + 0.5 * torch.rand(n, generator=g)) * tfx * z
        y = (torch.rand(n, generator=g) * 2 - 1) * 1.6 * tfy * z
        s = 0.3 * torch.exp(0.3 * torch.randn(n, 3, generator=g))
        parts.append((torch.stack([x, y, z], 1), s, torch.sigmoid(2.0 * torch.randn(n, 1, generator=g))))
    k = sum(p[0].shape[0] for p in parts)
    q = torch.randn(k, 4, generator=g)
    if not outside_clamp:
        # the GPU inputs: needles along the screen's x axis.  A needle turned in the image plane has b b ~ a0 c0, and float32
        # loses det0 = a0 c0 - b b to cancellation (tests/test_aa_cpu.py reports 7e-4 relative on the coefficient of such a
        # cloud); the GPU gradient test must only see inputs on which coef32 and coef64 agree to 1e-5
        q[n:2 * n] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    shs = torch.empty(k, cloud["shs"].shape[1], 3)
    shs[:, 0, :] = (torch.rand(k, 3, generator=g) - 0.5) / 0.28209479177387814
    shs[:, 1:, :] = 0.1 * torch.randn(k, shs.shape[1] - 1, 3, generator=g)
    return dict(means3D=torch.cat([cloud["means3D"]] + [p[0] for p in parts]).float().contiguous(),
                scales=torch.cat([cloud["scales"]] + [p[1] for p in parts]).float().contiguous(),
                rotations=torch.cat([cloud["rotations"], q / q.norm(dim=1, keepdim=True)]).float().contiguous(),
                opacities=torch.cat([cloud["opacities"]] + [p[2] for p in parts]).float().contiguous(),
                shs=torch.cat([cloud["shs"], shs]).float().contiguous())


def grad_case(i, outside_clamp=False):
    P, W, H, seed, sm = GRAD_CASES[i]
    cam, cloud = box_case(P, W, H, seed, sm)
    return cam, with_special_gaussians(cam, cloud, seed, outside_clamp)


def coef_of(cam, cloud, scale_modifier=1.0, cov3D_precomp=None, full=False):
    tfx, tfy = tan_fov(cam)
    if cov3D_precomp is not None:
        return aa_ref.coef32(cloud["means3D"], cam.world_view_transform, tfx, tfy, cam.image_width, cam.image_height,
                             cov3D_precomp=cov3D_precomp, full=full)
    return aa_ref.coef32(cloud["means3D"], cam.world_view_transform, tfx, tfy, cam.image_width, cam.image_height,
                         cloud["scales"], cloud["rotations"], scale_modifier, full=full)


def prescaled(cloud, coef):
    """The cloud with opacities `opacity * coef` (one float32 product, as preprocess forms the record's opacity)."""
    out = dict(cloud)
    out["opacities"] = torch.from_numpy((cloud["opacities"].numpy()[:, 0] * coef.astype(np.float32)).astype(np.float32)[:, None])
    return out


OFF_CASE = (6_000, 160, 128, 4, 0.6)


def render_off_case(device):
    """Colour, depth, radii and all gradients of the seeded "off is off" view (exact mode), as numpy arrays."""
    from luciddreamer_amd import config
    from tests import helpers as hp
    P, W, H, seed, sm = OFF_CASE
    cam, cloud = box_case(P, W, H, seed, sm)
    config.set_async(False)
    try:
        out = hp.run_hip(cloud, cam, 3, torch.tensor([0.1, 0.2, 0.3]), device, synthetic.upstream_grad(H, W))
    finally:
        config.set_async(True)
    res = dict(color=out["color"], depth=out["depth"], radii=out["radii"])
    res.update({"grad_" + k: v for k, v in out["grads"].items()})
    return res


if __name__ == "__main__":
    np.savez(sys.argv[1], **render_off_case(torch.device("cuda:0")))
