"""Differentiable alpha output on the GPU (return_alpha -> lr_render_alpha, lr_view_backward with dL_dalpha).

The forward's alpha against the float64 restatement tests/grad_oracle.py, gradients of losses on alpha (alone, and with
colour and depth mode) against its autograd, on every blend-backward shape and variant that reaches the alpha-mode kernels, a
C3-size consistency check (list segments against whole lists, against the two-render workaround, linearity), the bit guarantees,
memory, and ViewStreams.run_view with an alpha-requesting forward."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from luciddreamer_amd import _lib, cameras, config, synthetic
from tests import grad_oracle, helpers as hp

pytestmark = pytest.mark.gpu

NAMES_SH = ["means2D", "opacity", "means3D", "sh", "scales", "rotations"]
NAMES_PRE = ["means2D", "colors", "opacity", "means3D", "cov3D"]
RAW_PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


@pytest.fixture
def exact_mode():
    """Bit comparisons between calls: every forward in exact mode (async mode's binning bound can pick another shape)."""
    config.set_async(False)
    yield
    config.set_async(True)
    config.reset()


def _img(H, W, seed):
    return torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed))


def _settings(cam, bg, degree, dev, debug=False):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings
    tfx, tfy = hp.tan_fov(cam)
    c = cam.to(dev)
    return GaussianRasterizationSettings(cam.image_height, cam.image_width, tfx, tfy, bg.to(dev), 1.0, c.world_view_transform,
                                         c.full_proj_transform, degree, c.camera_center, False, debug)


def _run(cloud, cam, degree, bg, dev, gc=None, gd=None, ga=None, return_alpha=True, debug=False, colors_precomp=None,
         cov3D_precomp=None):
    """GaussianRasterizer(return_alpha) on fresh leaves; loss <gc, color> + <gd, depth> + <ga, alpha> (terms left out when
    None).  Returns images and the gradients in the oracle's naming."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizer
    d = lambda t: None if t is None else t.detach().to(dev).requires_grad_(True)
    m3, op = d(cloud["means3D"]), d(cloud["opacities"])
    sc = None if cov3D_precomp is not None else d(cloud["scales"])
    rot = None if cov3D_precomp is not None else d(cloud["rotations"])
    cov, cols = d(cov3D_precomp), d(colors_precomp)
    shs = d(cloud["shs"]) if colors_precomp is None else None
    m2 = torch.zeros_like(m3, requires_grad=True)
    out = GaussianRasterizer(_settings(cam, bg, degree, dev, debug))(
        means3D=m3, means2D=m2, opacities=op, shs=shs, colors_precomp=cols, scales=sc, rotations=rot, cov3D_precomp=cov,
        return_alpha=return_alpha)
    res = dict(color=out[0].detach().cpu(), radii=out[1].detach().cpu(), depth=out[2].detach().cpu())
    if return_alpha:
        res["alpha"] = out[3].detach().cpu()
    loss = None
    for t, g in ((out[0], gc), (out[2], gd), (out[3] if return_alpha else None, ga)):
        if g is not None:
            term = (t * g.to(dev)).sum()
            loss = term if loss is None else loss + term
    if loss is not None:
        loss.backward()
        P = m3.shape[0]
        z = lambda t, shape: np.zeros(shape, np.float32) if (t is None or t.grad is None) else t.grad.cpu().numpy()
        res["grads"] = dict(means2D=z(m2, (P, 3)), colors=z(cols, (P, 3)), opacity=z(op, (P, 1)), means3D=z(m3, (P, 3)),
                            cov3D=z(cov, (P, 6)), sh=z(shs, tuple(cloud["shs"].shape)), scales=z(sc, (P, 3)),
                            rotations=z(rot, (P, 4)))
    return res


def _oracle(cloud, cam, degree, bg, gc=None, gd=None, ga=None, colors_precomp=None, cov3D_precomp=None):
    leaf = lambda t: None if t is None else t.detach().double().clone().requires_grad_(True)
    m3, op = leaf(cloud["means3D"]), leaf(cloud["opacities"])
    sc = None if cov3D_precomp is not None else leaf(cloud["scales"])
    rot = None if cov3D_precomp is not None else leaf(cloud["rotations"])
    cov, cols = leaf(cov3D_precomp), leaf(colors_precomp)
    shs = leaf(cloud["shs"]) if colors_precomp is None else None
    m2 = torch.zeros_like(m3, requires_grad=True)
    tfx, tfy = hp.tan_fov(cam)
    col, dep, alpha, radii = grad_oracle.render(
        m3, op, cam.world_view_transform, cam.full_proj_transform, cam.camera_center, tfx, tfy, cam.image_height,
        cam.image_width, bg, scales=sc, rotations=rot, cov3D_precomp=cov, shs=shs, degree=degree, colors_precomp=cols, means2D=m2,
        alpha=True)
    res = dict(color=col.detach(), depth=dep.detach(), alpha=alpha.detach(), radii=radii)
    loss = None
    for t, g in ((col, gc), (dep, gd), (alpha, ga)):
        if g is not None:
            term = (t * g.double()).sum()
            loss = term if loss is None else loss + term
    if loss is not None:
        loss.backward()
        P = m3.shape[0]
        z = lambda t, shape: np.zeros(shape) if (t is None or t.grad is None) else t.grad.numpy()
        res["grads"] = dict(means2D=z(m2, (P, 3)), colors=z(cols, (P, 3)), opacity=z(op, (P, 1)), means3D=z(m3, (P, 3)),
                            cov3D=z(cov, (P, 6)), sh=z(shs, tuple(cloud["shs"].shape)), scales=z(sc, (P, 3)),
                            rotations=z(rot, (P, 4)))
    return res


def _check(dev, cloud, cam, degree, with_color_depth, names=NAMES_SH, debug=False, **kw):
    """Gradients of <ga, alpha> (+ <gc, color> + <gd, depth> with the depth switch on) against the oracle."""
    H, W = cam.image_height, cam.image_width
    bg = torch.zeros(3)
    ga = _img(H, W, 21)
    gc, gd = (synthetic.upstream_grad(H, W), _img(H, W, 22)) if with_color_depth else (None, None)
    ref = _oracle(cloud, cam, degree, bg, gc, gd, ga, **kw)
    if with_color_depth:
        config.set_depth_gradient(True)
    try:
        hip = _run(cloud, cam, degree, bg, dev, gc, gd, ga, debug=debug, **kw)
    finally:
        config.set_depth_gradient(False)
    assert float(np.abs(hip["grads"]["opacity"]).max()) > 0.0
    return hp.compare_grads(hip["grads"], ref["grads"], names=names)


# ---- forward ---------------------------------------------------------------------------------------------------------
def test_alpha_forward_matches_oracle_and_leaves_the_other_outputs_alone(hip_device, exact_mode):
    """Fails without the feature: return_alpha does not exist there."""
    W, H = 160, 128
    cam, cloud = hp.box_setup(6_000, W, H)
    bg = torch.tensor([0.0, 0.1, 0.2])
    ref = _oracle(cloud, cam, 3, bg)
    hip = _run(cloud, cam, 3, bg, hip_device)
    plain = _run(cloud, cam, 3, bg, hip_device, return_alpha=False)
    # float32 T_final against float64, off the pixels the C oracle flags as sitting on a discrete threshold (as the colour's
    # bar, helpers.compare_forward): the tolerance of the colour, of which alpha is the coverage channel
    fragile = torch.from_numpy(hp.run_oracle(cloud, cam, 3, bg)["res"].stage()["fragile"] != 0)
    diff = (hip["alpha"].double() - ref["alpha"]).abs()[0]
    assert int(fragile.sum()) <= max(8, hp.FRAGILE_FRAC * fragile.numel())
    err = float(diff[~fragile].max())
    assert err <= hp.COLOR_ATOL, err
    assert float(hip["alpha"].min()) >= 0.0 and float(hip["alpha"].max()) <= 1.0
    for k in ("color", "depth", "radii"):
        assert torch.equal(hip[k], plain[k]), k


def test_alpha_of_an_empty_cloud_and_of_an_async_rerender(hip_device):
    """P = 0: zeros.  Async mode with the verify policy and a binning buffer far too small: the view is rendered again, and
    alpha is that of the returned forward -- equal to an exact-mode render's."""
    W, H = 128, 96
    cam, cloud = hp.box_setup(5_000, W, H, seed=3)
    empty = {k: v[:0] for k, v in cloud.items()}
    assert float(_run(empty, cam, 1, torch.zeros(3), hip_device)["alpha"].abs().max()) == 0.0
    config.set_async(False)
    try:
        exact = _run(cloud, cam, 1, torch.zeros(3), hip_device)
    finally:
        config.set_async(True)
        config.reset()
    config.set_async(True, headroom=1.0, warm_calls=1)
    try:
        with torch.no_grad():
            _run(cloud, cam, 1, torch.zeros(3), hip_device)
        key = next(iter(config._hwm))
        config._hwm[key] = 64                                # the next forward overflows and is rendered again
        got = _run(cloud, cam, 1, torch.zeros(3), hip_device)
    finally:
        config.reset()
        config.set_async(True)
    assert torch.equal(got["color"], exact["color"])
    assert torch.equal(got["alpha"], exact["alpha"])


# ---- gradients against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 3])
@pytest.mark.parametrize("with_color_depth", [False, True], ids=["alpha_only", "color_depth_alpha"])
def test_alpha_loss_matches_oracle(hip_device, degree, with_color_depth):
    W, H = 160, 128
    cam, cloud = hp.box_setup(6_000, W, H)
    _check(hip_device, cloud, cam, degree, with_color_depth)


@pytest.mark.parametrize("with_color_depth", [False, True], ids=["alpha_only", "color_depth_alpha"])
def test_alpha_loss_precomputed_colors_and_cov(hip_device, with_color_depth):
    from oracle import torch_oracle
    W, H = 128, 96
    cam, cloud = hp.box_setup(4_000, W, H)
    cov = torch_oracle.cov3d_from_scale_rot(cloud["scales"].double(), 1.0, cloud["rotations"].double()).float()
    cols = torch.rand(4_000, 3, generator=torch.Generator().manual_seed(5))
    _check(hip_device, cloud, cam, 0, with_color_depth, names=NAMES_PRE, colors_precomp=cols, cov3D_precomp=cov)


@pytest.mark.parametrize("with_color_depth", [False, True], ids=["alpha_only", "color_depth_alpha"])
def test_alpha_loss_lists_longer_than_a_segment(hip_device, with_color_depth):
    """20 k large splats on 8 x 8 tiles: lists of several 256-instance segments, so alpha mode runs listed segments and their
    mid-list starts (T_final / T_ck); depth + alpha walks whole lists."""
    W, H = 128, 128
    cam, cloud = hp.box_setup(20_000, W, H, scale_mult=2.0)
    plain = _run(cloud, cam, 1, torch.zeros(3), hip_device, return_alpha=False)
    assert float((plain["radii"] > 0).sum()) / 64 > 256
    _check(hip_device, cloud, cam, 1, with_color_depth)


@pytest.mark.parametrize("with_color_depth", [False, True], ids=["alpha_only", "color_depth_alpha"])
def test_alpha_loss_on_the_one_wave_per_tile_shape(hip_device, exact_mode, with_color_depth):
    """An image above 3072 tiles (1040 x 768 = 3120): the one-wave-per-tile blend backward in alpha mode (depth + alpha: the
    depth-mode kernel).  Against the float64 oracle at the full-size bar of 1e-3 of each tensor's maximum (float32 rounding over
    3120 tiles: the depth-mode and alpha-mode kernels both land within 5e-4 of it on the same Gaussian); alpha alone also against
    the two-render workaround on the same shape (default kernels, colours 1, background 0) at 1e-4."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizer
    W, H = 1040, 768
    P = 3_000
    cam, cloud = hp.box_setup(P, W, H, seed=9)
    bg = torch.zeros(3)
    ga = _img(H, W, 21)
    gc, gd = (synthetic.upstream_grad(H, W), _img(H, W, 22)) if with_color_depth else (None, None)
    ref = _oracle(cloud, cam, 1, bg, gc, gd, ga)
    config.set_depth_gradient(with_color_depth)
    try:
        hip = _run(cloud, cam, 1, bg, hip_device, gc, gd, ga)
    finally:
        config.set_depth_gradient(False)
    assert _lib.last_launch_shapes()[1] == ("half" if with_color_depth else "tile")
    hp.compare_grads(hip["grads"], ref["grads"], names=NAMES_SH, rtol=1e-3)
    if with_color_depth:
        return
    d = lambda t: t.detach().to(hip_device).requires_grad_(True)
    m3, op, sc, rot = d(cloud["means3D"]), d(cloud["opacities"]), d(cloud["scales"]), d(cloud["rotations"])
    m2 = torch.zeros_like(m3, requires_grad=True)
    col = GaussianRasterizer(_settings(cam, bg, 1, hip_device))(means3D=m3, means2D=m2, opacities=op, scales=sc, rotations=rot,
                                                                colors_precomp=torch.ones(P, 3, device=hip_device))[0]
    assert _lib.last_launch_shapes()[1] is not None
    (col[0:1] * ga.to(hip_device)).sum().backward()
    two = dict(means2D=m2.grad.cpu().numpy(), opacity=op.grad.cpu().numpy(), means3D=m3.grad.cpu().numpy(),
               scales=sc.grad.cpu().numpy(), rotations=rot.grad.cpu().numpy())
    hp.compare_grads(hip["grads"], two, names=list(two))


@pytest.mark.parametrize("mode", ["strict", "debug", "fused"])
def test_alpha_loss_variants(hip_device, mode):
    W, H = 128, 96
    cam, cloud = hp.box_setup(4_000, W, H, seed=2)
    kw = {}
    if mode == "strict":
        config.set_strict_parity(True)
    elif mode == "debug":
        kw["debug"] = True
    else:
        config.set_fused_grad_accumulation(True)
    try:
        _check(hip_device, cloud, cam, 2, True, **kw)
        _check(hip_device, cloud, cam, 2, False, **kw)
    finally:
        config.set_strict_parity(False)
        config.set_fused_grad_accumulation(False)


def test_fused_accumulation_adds_the_alpha_gradient(hip_device):
    """Under fused accumulation a leaf's existing .grad receives += from the alpha-mode kernels (accumulate mode)."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizer
    W, H = 128, 96
    cam, cloud = hp.box_setup(4_000, W, H, seed=4)
    rs = _settings(cam, torch.zeros(3), 1, hip_device)
    p = {k: cloud[k].to(hip_device).clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    ga = _img(H, W, 8).to(hip_device)

    def once():
        m2 = torch.zeros_like(p["means3D"], requires_grad=True)
        alpha = GaussianRasterizer(rs)(means3D=p["means3D"], means2D=m2, opacities=p["opacities"], shs=p["shs"],
                                       scales=p["scales"], rotations=p["rotations"], return_alpha=True)[3]
        (alpha * ga).sum().backward()

    once()
    first = {k: v.grad.clone() for k, v in p.items()}
    config.set_fused_grad_accumulation(True)
    try:
        once()
    finally:
        config.set_fused_grad_accumulation(False)
    for k, v in p.items():
        if k == "shs":
            assert float(first[k].abs().max()) == 0.0                # colours get nothing from alpha
        else:
            assert float(first[k].abs().max()) > 0.0, k
        torch.testing.assert_close(v.grad, 2 * first[k], rtol=1e-5, atol=1e-7 * float(first[k].abs().max()) + 1e-30)


@pytest.mark.parametrize("with_depth", [False, True], ids=["color_alpha", "color_depth_alpha"])
def test_raw_path_matches_activated_path(hip_device, with_depth):
    """render_raw (the raw node, lr_view_backward with raw = 1 and dL_dalpha) = render on the activated tensors followed by autograd through
    exp / normalize / sigmoid, for a loss on colour, alpha (and depth)."""
    from luciddreamer_amd.gaussian_renderer import GaussianCloud, render, render_raw
    W, H = 256, 160
    c = synthetic.make_cloud(20_000, "band", 3)
    cam = cameras.rotate360_path(W, H, n_views=12)[2].to(hip_device)
    gc, gd, ga = synthetic.upstream_grad(H, W).to(hip_device), _img(H, W, 9).to(hip_device), _img(H, W, 10).to(hip_device)
    grads = []
    config.set_depth_gradient(with_depth)
    try:
        for fn in (render, render_raw):
            pc = GaussianCloud(c["means3D"].to(hip_device), c["scales"].to(hip_device), c["rotations"].to(hip_device),
                               c["opacities"].to(hip_device), c["shs"].to(hip_device), active_sh_degree=3)
            out = fn(cam, pc, return_alpha=True)
            loss = (out["render"] * gc).sum() + (out["alpha"] * ga).sum()
            if with_depth:
                loss = loss + (out["depth"] * gd).sum()
            loss.backward()
            grads.append({"viewspace": out["viewspace_points"].grad, **{n: getattr(pc, n).grad for n in RAW_PARAMS}})
    finally:
        config.set_depth_gradient(False)
    for k in grads[0]:
        a, b = grads[0][k], grads[1][k]
        scale = float(a.abs().max())
        assert scale > 0.0, k
        assert float((a - b).abs().max()) <= 1e-4 * scale, (k, float((a - b).abs().max()), scale)


def test_render_only_and_install_pass_alpha_through(hip_device):
    from luciddreamer_amd.gaussian_renderer import GaussianCloud, render, render_raw
    W, H = 128, 96
    c = synthetic.make_cloud(5_000, "band", 4)
    cam = cameras.rotate360_path(W, H, n_views=12)[0].to(hip_device)
    pc = GaussianCloud(c["means3D"].to(hip_device), c["scales"].to(hip_device), c["rotations"].to(hip_device),
                       c["opacities"].to(hip_device), c["shs"].to(hip_device), active_sh_degree=1)
    a = render(cam, pc, return_alpha=True)
    b = render_raw(cam, pc, render_only=True, return_alpha=True)
    assert set(b) == {"render", "depth", "alpha"} and "alpha" not in render(cam, pc)
    assert float((a["alpha"] - b["alpha"]).detach().abs().max()) <= 1e-6
    # install()'s render wrapper passes the keyword through: to the raw path, and -- for a call the reference's own render
    # would take (override_color), which has no such keyword -- to this package's render
    from luciddreamer_amd import dropin

    def reference_render(*args, **kw):
        raise AssertionError("the reference's render cannot return alpha")
    ns = SimpleNamespace(render=reference_render)
    opt = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    h = dropin.install(ns, None, None, losses=False, adam=False, stats=False)
    try:
        out = ns.render(cam, pc, opt, torch.zeros(3, device=hip_device), return_alpha=True)
        over = ns.render(cam, pc, opt, torch.zeros(3, device=hip_device), override_color=torch.ones_like(pc._xyz),
                         return_alpha=True)
    finally:
        dropin.uninstall(h)
    assert float((out["alpha"] - b["alpha"]).abs().max()) <= 1e-6
    assert float((over["alpha"] - b["alpha"]).abs().max()) <= 1e-6


def test_armed_fused_step_takes_the_alpha_gradient(hip_device):
    """The armed FusedAdam (raw node's no-zero-fill backward + masked step) with a colour + alpha loss: the same parameter bits
    as backward + step()."""
    from tests.test_gpu_optim import _adam_for, _two_clouds
    from luciddreamer_amd.gaussian_renderer import render_raw
    W, H = 320, 192
    a, b = _two_clouds(40_000, hip_device)
    for cl in (a, b):
        for n in RAW_PARAMS:
            setattr(cl, n, nn.Parameter(getattr(cl, n).detach()))
    opt_a, opt_b = _adam_for(a), _adam_for(b)
    cams = [c.to(hip_device) for c in cameras.rotate360_path(W, H, n_views=12)]
    bg = torch.zeros(3, device=hip_device)
    gen = torch.Generator().manual_seed(13)
    for it in range(4):
        cam = cams[(5 * it) % 12]
        g = torch.randn(3, H, W, generator=gen).to(hip_device)
        ga = torch.randn(1, H, W, generator=gen).to(hip_device)
        pa = render_raw(cam, a, bg_color=bg, return_alpha=True)
        ((pa["render"] * g).sum() + (pa["alpha"] * ga).sum()).backward()
        opt_a.step()
        opt_a.zero_grad(set_to_none=True)
        assert opt_b.arm_fused_backward()
        pb = render_raw(cam, b, bg_color=bg, return_alpha=True)
        ((pb["render"] * g).sum() + (pb["alpha"] * ga).sum()).backward()
        assert all(getattr(b, n).grad is None for n in RAW_PARAMS)
        opt_b.step()
        opt_b.zero_grad(set_to_none=True)
        assert torch.equal(pa["viewspace_points"].grad, pb["viewspace_points"].grad), it
        for n in RAW_PARAMS:
            assert torch.equal(getattr(a, n), getattr(b, n)), (it, n)


# ---- C3 size ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3(hip_device):
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    W, H = 1920, 1080
    c = synthetic.make_cloud(1_000_000, "band", 0)
    cam = cameras.rotate360_path(W, H, n_views=30)[3].to(hip_device)
    pc = GaussianCloud(c["means3D"].to(hip_device), c["scales"].to(hip_device), c["rotations"].to(hip_device),
                       c["opacities"].to(hip_device), c["shs"].to(hip_device), active_sh_degree=3)
    return SimpleNamespace(W=W, H=H, cam=cam, pc=pc, ga=_img(H, W, 14).to(hip_device),
                           gc=synthetic.upstream_grad(H, W).to(hip_device))


def _c3_grads(c3, wc=0.0, wa=1.0, override_color=None, bg=None, use="alpha"):
    from luciddreamer_amd.gaussian_renderer import render
    for n in RAW_PARAMS:
        getattr(c3.pc, n).grad = None
    out = render(c3.cam, c3.pc, bg_color=bg, override_color=override_color, return_alpha=use == "alpha")
    loss = (out["render"] * c3.gc).sum() * wc if wc else 0.0
    if use == "alpha":
        loss = loss + (out["alpha"] * c3.ga).sum() * wa
    else:                                                    # the two-render workaround: channel 0 of a coverage render
        loss = loss + (out["render"][0:1] * c3.ga).sum() * wa
    loss.backward()
    g = {"viewspace": out["viewspace_points"].grad.clone()}
    for n in RAW_PARAMS:
        t = getattr(c3.pc, n).grad
        g[n] = torch.zeros_like(getattr(c3.pc, n)) if t is None else t.clone()
    return g


def _close(a, b, k, tol=1e-4):
    scale = float(b.abs().max())
    assert scale > 0.0, k
    err = float((a - b).abs().max())
    assert bool(torch.isfinite(a).all()) and err <= tol * scale, (k, err, scale)


def test_c3_segments_match_whole_lists(hip_device, exact_mode, c3):
    seg = _c3_grads(c3)
    _lib.tune_set("bwd_seg", 0)
    try:
        whole = _c3_grads(c3)
    finally:
        _lib.tune_set("bwd_seg", -1)
    for k in seg:
        if k in ("_features_dc", "_features_rest"):
            assert float(seg[k].abs().max()) == 0.0 and float(whole[k].abs().max()) == 0.0, k
            continue
        _close(seg[k], whole[k], k)


def test_c3_matches_the_two_render_workaround(hip_device, exact_mode, c3):
    """colors_precomp = ones, background 0, default kernels, channel 0: the same geometric gradients to rounding."""
    got = _c3_grads(c3)
    ones = torch.ones_like(c3.pc._xyz)
    ref = _c3_grads(c3, override_color=ones, bg=torch.zeros(3, device=ones.device), use="two_render")
    for k in ("viewspace", "_xyz", "_opacity", "_scaling", "_rotation"):
        _close(got[k], ref[k], k)


def test_c3_is_linear_and_finite(hip_device, exact_mode, c3):
    both, col, alp = _c3_grads(c3, 1.0, 1.0), _c3_grads(c3, 1.0, 0.0), _c3_grads(c3, 0.0, 1.0)
    twice = _c3_grads(c3, 0.0, 2.0)
    assert float(alp["_xyz"].abs().max()) > 0.0
    for k in both:
        assert bool(torch.isfinite(both[k]).all()) and bool(torch.isfinite(alp[k]).all()), k
        scale = float(both[k].abs().max())
        assert float((both[k] - (col[k] + alp[k])).abs().max()) <= 1e-4 * scale + 1e-30, k
        assert float((twice[k] - 2 * alp[k]).abs().max()) <= 1e-5 * float(twice[k].abs().max()) + 1e-30, k


# ---- bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("debug", [False, True], ids=["compiled", "debug"])
def test_alpha_requested_but_unused_is_todays_bits(hip_device, exact_mode, debug):
    W, H = 160, 96
    cam, cloud = hp.box_setup(5_000, W, H, seed=6)
    gc = synthetic.upstream_grad(H, W)
    bg = torch.zeros(3)
    plain = _run(cloud, cam, 3, bg, hip_device, gc, return_alpha=False, debug=debug)
    unused = _run(cloud, cam, 3, bg, hip_device, gc, return_alpha=True, debug=debug)
    for k in plain["grads"]:
        np.testing.assert_array_equal(unused["grads"][k], plain["grads"][k], err_msg=k)


def test_alpha_mode_is_bit_repeatable(hip_device, exact_mode):
    W, H = 256, 192
    cam, cloud = hp.box_setup(20_000, W, H, seed=8, scale_mult=1.5)
    gc, ga = synthetic.upstream_grad(H, W), _img(H, W, 12)
    a = _run(cloud, cam, 3, torch.zeros(3), hip_device, gc, ga=ga)
    b = _run(cloud, cam, 3, torch.zeros(3), hip_device, gc, ga=ga)
    for k in a["grads"]:
        np.testing.assert_array_equal(a["grads"][k], b["grads"][k], err_msg=k)
    assert torch.equal(a["alpha"], b["alpha"])


@pytest.mark.parametrize("path", ["compiled", "debug", "raw"])
def test_alpha_mode_frees_its_nodes(hip_device, exact_mode, path):
    """Forward + backward with a loss on alpha, outputs dropped, the cyclic GC off: device memory does not grow."""
    import gc
    from luciddreamer_amd.gaussian_renderer import GaussianCloud, render, render_raw
    W, H = 256, 192
    c = synthetic.make_cloud(20_000, "band", 5)
    cam = cameras.rotate360_path(W, H, n_views=12)[1].to(hip_device)
    pc = GaussianCloud(c["means3D"].to(hip_device), c["scales"].to(hip_device), c["rotations"].to(hip_device),
                       c["opacities"].to(hip_device), c["shs"].to(hip_device), active_sh_degree=1)
    gc_img, ga = synthetic.upstream_grad(H, W).to(hip_device), _img(H, W, 15).to(hip_device)
    opt = SimpleNamespace(debug=path == "debug", compute_cov3D_python=False, convert_SHs_python=False)
    fn = render_raw if path == "raw" else render

    def step():
        out = fn(cam, pc, opt, return_alpha=True)
        loss = (out["render"] * gc_img).sum() + (out["alpha"] * ga).sum()
        loss.backward()
        del out, loss
        for t in pc.parameters():
            t.grad = None
    was = gc.isenabled()
    gc.disable()
    try:
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(hip_device)
        for _ in range(6):
            step()
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated(hip_device) - before
    finally:
        if was:
            gc.enable()
    assert grown < 256 * 1024, grown


# ---- ViewStreams.run_view --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [True, False], ids=["fused_path", "engine_path"])
def test_run_view_with_an_alpha_requesting_forward_equals_autograd(hip_device, direct):
    """forward_fn asks for alpha and returns the colour: never the direct view-step route; the gradients are the autograd
    route's for the same colour gradient."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizer
    from luciddreamer_amd import parallel
    P, W, H = 30_000, 320, 180
    cloud = synthetic.make_cloud(P, "band", 4)
    cams = [c.to(hip_device) for c in cameras.rotate360_path(W, H, n_views=4)]
    g = synthetic.upstream_grad(H, W).to(hip_device)
    bg = torch.zeros(3)

    def run(stream_path):
        leaf = {k: v.to(hip_device).requires_grad_(True) for k, v in cloud.items()}
        grads = parallel.FlatGrads(list(leaf.values()))
        m2d = torch.zeros(P, 3, device=hip_device, requires_grad=True)
        m2d.grad = torch.zeros_like(m2d)
        config.set_async(False)
        config.set_fused_grad_accumulation(stream_path)
        try:
            def fwd(c):
                col, _, _, alpha = GaussianRasterizer(_settings(c, bg, 3, hip_device))(
                    means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"], shs=leaf["shs"], scales=leaf["scales"],
                    rotations=leaf["rotations"], return_alpha=True)
                assert alpha.requires_grad
                return col
            if stream_path:
                pipe = parallel.ViewStreams(hip_device, 2, direct=direct)
                pipe.begin_step()
                for c in cams:
                    pipe.run_view(lambda c=c: fwd(c), grad_output=g)
                pipe.end_step()
            else:
                for c in cams:
                    (fwd(c) * g).sum().backward()
            torch.cuda.synchronize()
        finally:
            config.set_fused_grad_accumulation(False)
            config.set_async(True)
            config.reset()
        for v, p in zip(grads.views, leaf.values()):
            if p.grad.data_ptr() != v.data_ptr():
                v.copy_(p.grad)
        return grads.flat.clone(), m2d.grad.clone()
    f_ref, m_ref = run(False)
    f, m = run(True)
    _close(f, f_ref, "flat", tol=2e-5)
    _close(m, m_ref, "means2D", tol=2e-5)
