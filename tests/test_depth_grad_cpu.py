"""Differentiable depth output (config.set_depth_gradient, lr_view_backward with dL_depths and depth_image): the contract's CPU side.

tests/grad_oracle.py restates oracle/torch_oracle.render without the two detach() calls on depth; these tests check that
restatement against torch_oracle (colour gradients unchanged) and against float64 central differences (the depth gradient is
the true derivative of what the forward outputs), and that the switch and the C-ABI entry points exist."""
import os
import re

import torch

from luciddreamer_amd import cameras, synthetic
from oracle import torch_oracle
from tests import grad_oracle, helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(P, W, H, seed):
    cam = cameras.identity_camera(W, H)
    cloud = synthetic.make_cloud(P, "box", seed, sh_coeffs=16)
    return cam, cloud


def _params(cloud, opacity=None):
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    p = dict(means3D=leaf(cloud["means3D"]), opacities=leaf(cloud["opacities"] if opacity is None else opacity),
             scales=leaf(cloud["scales"]), rotations=leaf(cloud["rotations"]), shs=leaf(cloud["shs"]))
    p["means2D"] = torch.zeros_like(p["means3D"], requires_grad=True)
    return p


def _render(mod, cam, p, degree, bg, **kw):
    tfx, tfy = hp.tan_fov(cam)
    return mod.render(p["means3D"], p["opacities"], cam.world_view_transform, cam.full_proj_transform, cam.camera_center,
                      tfx, tfy, cam.image_height, cam.image_width, bg, scales=p["scales"], rotations=p["rotations"],
                      shs=p["shs"], degree=degree, means2D=p["means2D"], **kw)


def test_detached_depth_restatement_matches_torch_oracle():
    """With depth detached again, the restated render loop IS torch_oracle's: same images, colour gradients within 1e-12."""
    cam, cloud = _scene(300, 64, 48, 3)
    bg = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    gc = torch.randn(3, 48, 64, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out = {}
    for name, mod, kw in (("ref", torch_oracle, {}), ("new", grad_oracle, dict(detach_depth=True))):
        p = _params(cloud)
        col, dep, radii = _render(mod, cam, p, 3, bg, **kw)
        (col * gc).sum().backward()
        out[name] = (col.detach(), dep.detach(), radii, {k: v.grad.clone() for k, v in p.items()})
    (c0, d0, r0, g0), (c1, d1, r1, g1) = out["ref"], out["new"]
    assert torch.equal(c0, c1) and torch.equal(d0, d1) and torch.equal(r0, r1)
    for k in g0:
        assert float((g0[k] - g1[k]).abs().max()) <= 1e-12, k


def test_depth_gradient_matches_central_differences():
    """A depth-only loss on a tiny scene away from the discrete thresholds (opacities <= 0.6: alpha never reaches the 0.99
    clamp and T never the 1e-4 stop): the restatement's autograd gradient with respect to means3D, opacities, scales and
    rotations is the float64 central difference of the loss -- and it is not zero."""
    P, W, H = 10, 40, 32
    cam, cloud = _scene(P, W, H, 11)
    op = 0.25 + 0.35 * torch.rand(P, 1, generator=torch.Generator().manual_seed(4))
    cloud = dict(cloud)
    cloud["scales"] = cloud["scales"] * 4.0              # footprints of several pixels: most pixels see a few layers
    bg = torch.zeros(3, dtype=torch.float64)
    gd = torch.randn(1, H, W, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    p = _params(cloud, op)
    _, dep, radii = _render(grad_oracle, cam, p, 0, bg)
    assert int((radii > 0).sum()) >= 5 and float((dep != 0).double().mean()) > 0.2
    (dep * gd).sum().backward()

    def loss_at(name, flat_index, delta):
        q = {k: v.detach().clone() for k, v in p.items()}
        q[name].view(-1)[flat_index] += delta
        with torch.no_grad():
            _, d, _ = _render(grad_oracle, cam, q, 0, bg)
        return float((d * gd).sum())

    eps = 1e-6
    for name in ("means3D", "opacities", "scales", "rotations"):
        auto = p[name].grad.reshape(-1)
        assert float(auto.abs().max()) > 0.0, name
        num = torch.tensor([(loss_at(name, i, eps) - loss_at(name, i, -eps)) / (2 * eps) for i in range(auto.numel())],
                           dtype=torch.float64)
        err = float((num - auto).abs().max())
        assert err <= 1e-5 * max(1.0, float(auto.abs().max())), (name, err, float(auto.abs().max()))


def test_depth_gradient_switch_defaults_to_off():
    from luciddreamer_amd import config
    assert callable(config.set_depth_gradient)
    assert config.depth_gradient() is False
    config.set_depth_gradient(True)
    try:
        assert config.depth_gradient() is True
    finally:
        config.set_depth_gradient(False)
    assert config.depth_gradient() is False


def test_header_declares_the_depth_entry_points():
    text = open(os.path.join(ROOT, "include", "lucid_raster.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^int\s+lr_view_backward\s*\(const lr_backward_args\*[^;]*\);", text, flags=re.M)
    m = re.search(r"typedef struct lr_backward_args \{(.*?)\} lr_backward_args;", text, flags=re.S)
    assert m
    args = m.group(1)                                   # one struct for activated and raw mode
    assert "const float* dL_depths;" in args and "const float* depth_image;" in args
    from luciddreamer_amd import _lib
    names = [f[0] for f in _lib.BackwardArgs._fields_]
    assert "dL_depths" in names and "depth_image" in names
    assert "lr_view_backward" in _lib.EXPORTS
