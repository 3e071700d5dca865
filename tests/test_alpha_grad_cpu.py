"""Differentiable alpha output (return_alpha, lr_render_alpha / lr_view_backward with dL_dalpha): the contract's CPU side.

tests/grad_oracle.py restates the render loop with alpha = 1 - T_final as an output (alpha=True).  These tests check that
output against the same render without it (same colour, depth and radii), against the coverage render and against float64
central differences, the per-layer closed form d alpha_pix / d alpha_i = T_final / (1 - alpha_i), the blend backward's
recursion for the coverage channel (the start values of A the alpha-mode kernels use, whole lists and segment starts), and
that the new C-ABI entry points are declared and exported."""
import ctypes
import os
import re

import numpy as np
import torch

from luciddreamer_amd import cameras, synthetic
from tests import grad_oracle, helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(P, W, H, seed, scale_mult=1.0):
    cam = cameras.identity_camera(W, H)
    cloud = synthetic.make_cloud(P, "box", seed, sh_coeffs=16, scale_mult=scale_mult)
    return cam, cloud


def _params(cloud, opacity=None):
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    p = dict(means3D=leaf(cloud["means3D"]), opacities=leaf(cloud["opacities"] if opacity is None else opacity),
             scales=leaf(cloud["scales"]), rotations=leaf(cloud["rotations"]), shs=leaf(cloud["shs"]))
    p["means2D"] = torch.zeros_like(p["means3D"], requires_grad=True)
    return p


def _render(cam, p, degree, bg, **kw):
    tfx, tfy = hp.tan_fov(cam)
    return grad_oracle.render(p["means3D"], p["opacities"], cam.world_view_transform, cam.full_proj_transform,
                              cam.camera_center, tfx, tfy, cam.image_height, cam.image_width, bg, scales=p["scales"],
                              rotations=p["rotations"], shs=p["shs"], degree=degree, means2D=p["means2D"], **kw)


def test_colour_depth_radii_are_depth_oracle_s_and_alpha_is_coverage():
    """Colour, depth and radii bit-equal to the depth oracle's (the same render without alpha=True), and so are the colour
    gradients; alpha in [0, 1], 0 where nothing is drawn, equal to 1 - T_final -- which is also the coverage render (colours 1,
    background 0)."""
    cam, cloud = _scene(300, 64, 48, 3)
    bg = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    gc = torch.randn(3, 48, 64, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    p0, p1 = _params(cloud), _params(cloud)
    c0, d0, r0 = _render(cam, p0, 3, bg)
    c1, d1, a1, r1 = _render(cam, p1, 3, bg, alpha=True)
    assert torch.equal(c0, c1) and torch.equal(d0, d1) and torch.equal(r0, r1)
    (c0 * gc).sum().backward()
    (c1 * gc).sum().backward()
    for k in p0:
        assert torch.equal(p0[k].grad, p1[k].grad), k
    a1 = a1.detach()
    assert a1.shape == (1, 48, 64) and float(a1.min()) >= 0.0 and float(a1.max()) <= 1.0
    assert float((a1 == 0).double().mean()) > 0.0 and float(a1.max()) > 0.5       # holes and covered pixels both present
    # the coverage channel: colours 1, background 0
    tfx, tfy = hp.tan_fov(cam)
    q = _params(cloud)
    cov_img, _, _ = grad_oracle.render(q["means3D"], q["opacities"], cam.world_view_transform, cam.full_proj_transform,
                                       cam.camera_center, tfx, tfy, 48, 64, torch.zeros(3, dtype=torch.float64),
                                       scales=q["scales"], rotations=q["rotations"],
                                       colors_precomp=torch.ones(300, 3, dtype=torch.float64))
    assert float((cov_img[0:1].detach() - a1).abs().max()) <= 1e-12
    # 1 - T_final per pixel, from the applied layers
    _, _, a2, _, layers = _render(cam, _params(cloud), 3, bg, alpha=True, with_layers=True)
    for t in layers:
        ys, xs = t["pix"]
        inside = (ys < 48) & (xs < 64)
        assert torch.equal(a2.detach()[0, ys[inside], xs[inside]], (1.0 - t["T_fin"])[inside])


def test_alpha_gradient_matches_central_differences():
    """An alpha-only loss on a tiny scene away from the discrete thresholds (opacities <= 0.6: alpha never reaches the 0.99
    clamp and T never the 1e-4 stop): the restatement's autograd gradient is the float64 central difference, and not zero."""
    P, W, H = 10, 40, 32
    cam, cloud = _scene(P, W, H, 11)
    op = 0.25 + 0.35 * torch.rand(P, 1, generator=torch.Generator().manual_seed(4))
    cloud = dict(cloud)
    cloud["scales"] = cloud["scales"] * 4.0
    bg = torch.zeros(3, dtype=torch.float64)
    ga = torch.randn(1, H, W, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    p = _params(cloud, op)
    _, _, alpha, radii = _render(cam, p, 0, bg, alpha=True)
    assert int((radii > 0).sum()) >= 5 and float((alpha > 0).double().mean()) > 0.2
    (alpha * ga).sum().backward()

    def loss_at(name, flat_index, delta):
        q = {k: v.detach().clone() for k, v in p.items()}
        q[name].view(-1)[flat_index] += delta
        with torch.no_grad():
            _, _, a, _ = _render(cam, q, 0, bg, alpha=True)
        return float((a * ga).sum())

    eps = 1e-6
    for name in ("means3D", "opacities", "scales", "rotations", "means2D"):
        auto = p[name].grad.reshape(-1)
        if name == "means2D":
            auto = p[name].grad[:, :2].reshape(-1)                  # the z column of means2D is unused
            idx = [3 * (i // 2) + (i % 2) for i in range(auto.numel())]
        else:
            idx = list(range(auto.numel()))
        assert float(auto.abs().max()) > 0.0, name
        num = torch.tensor([(loss_at(name, i, eps) - loss_at(name, i, -eps)) / (2 * eps) for i in idx], dtype=torch.float64)
        err = float((num - auto).abs().max())
        assert err <= 1e-5 * max(1.0, float(auto.abs().max())), (name, err, float(auto.abs().max()))
    assert p["shs"].grad is None or float(p["shs"].grad.abs().max()) == 0.0      # colours get nothing from alpha


def test_per_layer_closed_form():
    """For L = alpha at one pixel, dL/dopacity_g = T_final / (1 - alpha_g) * alpha_g / opacity_g for every Gaussian g applied
    at that pixel (alpha_g = opacity_g G_g, unclamped here), 0 for the others."""
    P, W, H = 40, 32, 32
    cam, cloud = _scene(P, W, H, 5)
    op = 0.2 + 0.4 * torch.rand(P, 1, generator=torch.Generator().manual_seed(6))
    cloud = dict(cloud)
    cloud["scales"] = cloud["scales"] * 4.0
    bg = torch.zeros(3, dtype=torch.float64)
    _, _, alpha0, _, layers = _render(cam, _params(cloud, op), 0, bg, alpha=True, with_layers=True)
    checked = 0
    for t in layers:
        n_applied = t["contrib"].sum(dim=1)
        for k in torch.nonzero(n_applied >= 3).flatten()[:3].tolist():
            y, x = int(t["pix"][0][k]), int(t["pix"][1][k])
            p = _params(cloud, op)
            _, _, alpha, _ = _render(cam, p, 0, bg, alpha=True)
            alpha[0, y, x].backward()
            expect = torch.zeros(P, dtype=torch.float64)
            for j in torch.nonzero(t["contrib"][k]).flatten().tolist():
                g, a = int(t["ids"][j]), float(t["alpha"][k, j])
                expect[g] = float(t["T_fin"][k]) / (1.0 - a) * a / float(op[g])
            got = p["opacities"].grad.reshape(-1)
            assert float((got - expect).abs().max()) <= 1e-12 * max(1.0, float(expect.abs().max())), (y, x)
            checked += 1
    assert checked >= 3


def _kernel_recursion(a, c, bg, dL, g, seg_start=None):
    """The blend backward's per-pixel recursion (render_bwd.hip bwd_pixel), back to front over the applied layers, in float64,
    with the alpha-mode start values of A: returns dL/dalpha_i.  seg_start = s: the recursion starts at list position s, as a
    segment whose deep end is s does -- T = T_s, A = (final colour - colour so far).dL / T_s - g T_final / T_s."""
    n = len(a)
    T_before = np.cumprod(np.concatenate([[1.0], 1.0 - a]))       # T_before[i]: T in front of layer i; T_before[n] = T_final
    T_fin = T_before[n]
    out = np.zeros(n)
    if seg_start is None:
        hi, T, A = n, T_fin, float(bg @ dL) - g
    else:
        hi = seg_start
        final = sum(c[j] * a[j] * T_before[j] for j in range(n)) + T_fin * bg
        so_far = sum(c[j] * a[j] * T_before[j] for j in range(seg_start))
        T = T_before[seg_start]
        A = float((final - so_far) @ dL - g * T_fin) / T
    for i in range(hi - 1, -1, -1):
        T = T / (1.0 - a[i])
        d = float(c[i] @ dL) - A
        out[i] = T * d
        A = A + a[i] * d
    return out


def test_coverage_recursion_matches_autograd_whole_lists_and_segment_starts():
    """The algebra the alpha-mode kernels rely on: with A started at bg.dL - g (whole list) or at the segment start's colour
    share minus g T_final / T_ck, the unchanged per-layer recursion gives d/dalpha_i of colour.dL + g alpha_pix exactly."""
    gen = torch.Generator().manual_seed(9)
    for trial in range(20):
        n = 3 + trial % 9
        a = (0.02 + 0.9 * torch.rand(n, generator=gen, dtype=torch.float64)).requires_grad_(True)
        c = torch.rand(n, 3, generator=gen, dtype=torch.float64)
        bg = torch.rand(3, generator=gen, dtype=torch.float64)
        dL = torch.randn(3, generator=gen, dtype=torch.float64)
        g = float(torch.randn(1, generator=gen, dtype=torch.float64))
        T_before = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1.0 - a]), 0)
        colour = (c * (a * T_before[:n])[:, None]).sum(0) + T_before[n] * bg
        loss = colour @ dL + g * (1.0 - T_before[n])
        loss.backward()
        ref = a.grad.numpy()
        args = (a.detach().numpy(), c.numpy(), bg.numpy(), dL.numpy(), g)
        for s in [None] + list(range(1, n)):
            got = _kernel_recursion(*args, seg_start=s)
            hi = n if s is None else s
            np.testing.assert_allclose(got[:hi], ref[:hi], rtol=1e-10, atol=1e-12, err_msg=f"trial {trial}, segment start {s}")
        # and the closed form of alpha's own share
        np.testing.assert_allclose(_kernel_recursion(a.detach().numpy(), np.zeros((n, 3)), np.zeros(3), np.zeros(3), 1.0),
                                   float(T_before[n].detach()) / (1.0 - a.detach().numpy()), rtol=1e-12)


def test_header_declares_and_library_exports_the_alpha_entry_points():
    text = open(os.path.join(ROOT, "include", "lucid_raster.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^int\s+lr_view_backward\s*\(const lr_backward_args\*[^;]*\);", text, flags=re.M)
    m = re.search(r"typedef struct lr_backward_args \{(.*?)\} lr_backward_args;", text, flags=re.S)
    assert m                                            # one struct for activated and raw mode
    assert re.search(r"const float\* depth_image;\s*const float\* dL_dalpha;", m.group(1))
    m = re.search(r"^int\s+lr_render_alpha\s*\(([^;]*)\);", text, flags=re.M)
    assert m and "float* out_alpha" in m.group(1)
    from luciddreamer_amd import _lib, build
    L = ctypes.CDLL(build.build())
    for name in ("lr_view_backward", "lr_render_alpha"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
    names = [f[0] for f in _lib.BackwardArgs._fields_]
    assert names[names.index("depth_image") + 1] == "dL_dalpha"


def test_public_signatures_take_return_alpha():
    import inspect
    from luciddreamer_amd import _C, gaussian_renderer, rasterizer
    for fn in (rasterizer.GaussianRasterizer.forward, rasterizer.rasterize_gaussians, rasterizer.rasterize_gaussians_raw,
               gaussian_renderer.render, gaussian_renderer.render_raw):
        assert inspect.signature(fn).parameters["return_alpha"].default is False, fn
    for fn in (_C.rasterize_gaussians_backward, _C.rasterize_gaussians_raw_backward):
        assert inspect.signature(fn).parameters["dL_dout_alpha"].default is None, fn
