"""Differentiable depth output on the GPU (config.set_depth_gradient -> lr_view_backward with dL_depths and depth_image).

Gradients of losses on `depth` against the float64 restatement tests/grad_oracle.py (sizes bounded by that Python
oracle), the variants that reach the depth-mode kernels (strict parity, the Python debug node, fused accumulation, the raw
path, the armed optimizer step), the switch's bit-identity guarantees, repeatability, and a C3-size consistency check."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from luciddreamer_amd import cameras, config, synthetic
from tests import grad_oracle, helpers as hp

pytestmark = pytest.mark.gpu

NAMES_SH = ["means2D", "opacity", "means3D", "sh", "scales", "rotations"]
NAMES_PRE = ["means2D", "colors", "opacity", "means3D", "cov3D"]


@pytest.fixture
def depth_on():
    config.set_depth_gradient(True)
    yield
    config.set_depth_gradient(False)


@pytest.fixture
def exact_mode():
    """Bit comparisons between calls: every forward in exact mode.  (Async mode sizes the binning buffer from the calls seen
    before, and the bound it hands the backward can pick another blend-backward shape -- the same gradients, other bits.)"""
    config.set_async(False)
    yield
    config.set_async(True)
    config.reset()


def _upstream(H, W, seed):
    return torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed))


def _oracle(cloud, cam, degree, bg, gc, gd, colors_precomp=None, cov3D_precomp=None):
    """Gradients of sum(color * gc) + sum(depth * gd) by autograd through the depth-differentiable restatement."""
    leaf = lambda t: None if t is None else t.detach().double().clone().requires_grad_(True)
    m3, op = leaf(cloud["means3D"]), leaf(cloud["opacities"])
    sc = None if cov3D_precomp is not None else leaf(cloud["scales"])
    rot = None if cov3D_precomp is not None else leaf(cloud["rotations"])
    cov, cols = leaf(cov3D_precomp), leaf(colors_precomp)
    shs = leaf(cloud["shs"]) if colors_precomp is None else None
    m2 = torch.zeros_like(m3, requires_grad=True)
    tfx, tfy = hp.tan_fov(cam)
    col, dep, _ = grad_oracle.render(m3, op, cam.world_view_transform, cam.full_proj_transform, cam.camera_center, tfx, tfy,
                                     cam.image_height, cam.image_width, bg, scales=sc, rotations=rot, cov3D_precomp=cov,
                                     shs=shs, degree=degree, colors_precomp=cols, means2D=m2)
    ((col * gc.double()).sum() + (dep * gd.double()).sum()).backward()
    P = m3.shape[0]
    z = lambda t, shape: np.zeros(shape) if (t is None or t.grad is None) else t.grad.numpy()
    return dict(means2D=z(m2, (P, 3)), colors=z(cols, (P, 3)), opacity=z(op, (P, 1)), means3D=z(m3, (P, 3)),
                cov3D=z(cov, (P, 6)), sh=z(shs, tuple(cloud["shs"].shape)), scales=z(sc, (P, 3)), rotations=z(rot, (P, 4)))


def _check(hip_device, cloud, cam, degree, gc, gd, names=NAMES_SH, **kw):
    bg = torch.zeros(3)
    ref = _oracle(cloud, cam, degree, bg, gc, gd, **kw)
    hip = hp.run_hip(cloud, cam, degree, bg, hip_device, gc, grad_depth=gd, **kw)
    assert float(np.abs(hip["grads"]["means3D"]).max()) > 0.0
    return hp.compare_grads(hip["grads"], ref, names=names)


@pytest.mark.parametrize("degree", [0, 3])
@pytest.mark.parametrize("with_color", [False, True], ids=["depth_only", "color_and_depth"])
def test_depth_loss_matches_oracle(hip_device, depth_on, degree, with_color):
    """Fails without the feature: a depth-only loss gives zero gradients there (the reference's behaviour)."""
    W, H = 160, 128
    cam, cloud = hp.box_setup(6_000, W, H)
    gc = synthetic.upstream_grad(H, W) if with_color else torch.zeros(3, H, W)
    _check(hip_device, cloud, cam, degree, gc, _upstream(H, W, 3))


def test_depth_loss_dense_lists_longer_than_a_segment(hip_device, depth_on):
    """20 k large splats on 8 x 8 tiles: every tile's list is several 256-instance segments long (the default backward splits
    them; depth mode walks each tile's whole list)."""
    W, H = 128, 128
    cam, cloud = hp.box_setup(20_000, W, H, scale_mult=2.0)
    hip = hp.run_hip(cloud, cam, 1, torch.zeros(3), hip_device)
    radii = torch.from_numpy(hip["radii"]).float()
    assert float((radii > 0).sum()) / 64 > 256               # more Gaussians than a segment holds reach an average tile
    _check(hip_device, cloud, cam, 1, synthetic.upstream_grad(H, W), _upstream(H, W, 4))


def test_depth_loss_precomputed_colors_and_cov(hip_device, depth_on):
    from oracle import torch_oracle
    W, H = 128, 96
    cam, cloud = hp.box_setup(4_000, W, H)
    cov = torch_oracle.cov3d_from_scale_rot(cloud["scales"].double(), 1.0, cloud["rotations"].double()).float()
    cols = torch.rand(4_000, 3, generator=torch.Generator().manual_seed(5))
    _check(hip_device, cloud, cam, 0, synthetic.upstream_grad(H, W), _upstream(H, W, 5), names=NAMES_PRE,
           colors_precomp=cols, cov3D_precomp=cov)


@pytest.mark.parametrize("mode", ["strict", "debug", "fused"])
def test_depth_loss_variants(hip_device, depth_on, mode):
    """Strict parity (STRICT kernels), the Python autograd node (debug=True), and the switch for fused gradient accumulation
    (run_hip's leaves are fresh, so the kernels WRITE here; accumulate mode in depth mode is
    test_fused_accumulation_adds_the_depth_gradient)."""
    W, H = 128, 96
    cam, cloud = hp.box_setup(4_000, W, H, seed=2)
    gc, gd = synthetic.upstream_grad(H, W), _upstream(H, W, 6)
    kw = {}
    if mode == "strict":
        config.set_strict_parity(True)
    elif mode == "debug":
        kw["debug"] = True
    else:
        config.set_fused_grad_accumulation(True)
    try:
        bg = torch.zeros(3)
        ref = _oracle(cloud, cam, 2, bg, gc, gd)
        hip = hp.run_hip(cloud, cam, 2, bg, hip_device, gc, grad_depth=gd, **kw)
        hp.compare_grads(hip["grads"], ref, names=NAMES_SH)
    finally:
        config.set_strict_parity(False)
        config.set_fused_grad_accumulation(False)


def test_fused_accumulation_adds_the_depth_gradient(hip_device, depth_on):
    """Under fused accumulation a leaf's existing .grad receives += from the depth-mode kernels (accumulate mode)."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    W, H = 128, 96
    cam, cloud = hp.box_setup(4_000, W, H, seed=4)
    camd = cam.to(hip_device)
    tfx, tfy = hp.tan_fov(cam)
    rs = GaussianRasterizationSettings(H, W, tfx, tfy, torch.zeros(3, device=hip_device), 1.0, camd.world_view_transform,
                                       camd.full_proj_transform, 1, camd.camera_center, False, False)
    leaf = lambda k: cloud[k].to(hip_device).clone().requires_grad_(True)
    p = {k: leaf(k) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    gd = _upstream(H, W, 8).to(hip_device)

    def once():
        m2 = torch.zeros_like(p["means3D"], requires_grad=True)
        _, _, dep = GaussianRasterizer(rs)(means3D=p["means3D"], means2D=m2, opacities=p["opacities"], shs=p["shs"],
                                           scales=p["scales"], rotations=p["rotations"])
        (dep * gd).sum().backward()

    once()
    first = {k: v.grad.clone() for k, v in p.items()}
    config.set_fused_grad_accumulation(True)
    try:
        once()
    finally:
        config.set_fused_grad_accumulation(False)
    for k, v in p.items():
        assert float(first[k].abs().max()) > 0.0 or k == "shs", k
        torch.testing.assert_close(v.grad, 2 * first[k], rtol=1e-5, atol=1e-7 * float(first[k].abs().max()) + 1e-30)


def test_raw_path_matches_activated_path(hip_device, depth_on):
    """render_raw (the raw node, lr_view_backward with raw = 1, dL_depths and depth_image) = render on the activated tensors followed by autograd through
    exp / normalize / sigmoid, for a colour + depth loss."""
    from luciddreamer_amd.gaussian_renderer import GaussianCloud, render, render_raw
    W, H = 256, 160
    c = synthetic.make_cloud(20_000, "band", 3)
    cam = cameras.rotate360_path(W, H, n_views=12)[2].to(hip_device)
    gc, gd = synthetic.upstream_grad(H, W).to(hip_device), _upstream(H, W, 9).to(hip_device)
    grads = []
    for fn in (render, render_raw):
        pc = GaussianCloud(c["means3D"].to(hip_device), c["scales"].to(hip_device), c["rotations"].to(hip_device),
                           c["opacities"].to(hip_device), c["shs"].to(hip_device), active_sh_degree=3)
        out = fn(cam, pc)
        ((out["render"] * gc).sum() + (out["depth"] * gd).sum()).backward()
        grads.append({"viewspace": out["viewspace_points"].grad, **{n: getattr(pc, n).grad for n in
                      ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")}})
    for k in grads[0]:
        a, b = grads[0][k], grads[1][k]
        scale = float(a.abs().max())
        assert scale > 0.0, k
        assert float((a - b).abs().max()) <= 1e-4 * scale, (k, float((a - b).abs().max()), scale)


def _grads_of(hip_device, cloud, cam, gc, gd, use_depth=True):
    hip = hp.run_hip(cloud, cam, 3, torch.zeros(3), hip_device, gc, grad_depth=gd if use_depth else None)
    return hip["grads"]


def test_switch_off_and_unused_depth_are_todays_bits(hip_device, exact_mode):
    W, H = 160, 96
    cam, cloud = hp.box_setup(5_000, W, H, seed=6)
    gc, gd = synthetic.upstream_grad(H, W), _upstream(H, W, 10)
    off_depth_only = _grads_of(hip_device, cloud, cam, torch.zeros(3, H, W), gd)
    for k, v in off_depth_only.items():
        assert float(np.abs(v).max()) == 0.0, k                  # as today: the depth gradient is ignored
    off = _grads_of(hip_device, cloud, cam, gc, None, use_depth=False)
    config.set_depth_gradient(True)
    try:
        on_no_depth = _grads_of(hip_device, cloud, cam, gc, None, use_depth=False)
        on_zero_weight = _grads_of(hip_device, cloud, cam, gc, torch.zeros(1, H, W))    # depth in the loss, gradient zero
    finally:
        config.set_depth_gradient(False)
    for k in off:
        np.testing.assert_array_equal(on_no_depth[k], off[k], err_msg=k)
        np.testing.assert_allclose(on_zero_weight[k], off[k], rtol=0, atol=1e-6 * float(np.abs(off[k]).max()) + 1e-30,
                                   err_msg=k)


def test_depth_unused_in_loss_is_todays_bits(hip_device, depth_on, exact_mode):
    """Switch on, depth output not used by the loss: grad_depth arrives as None -> the default kernels, the same bits."""
    W, H = 160, 96
    cam, cloud = hp.box_setup(5_000, W, H, seed=6)
    gc = synthetic.upstream_grad(H, W)
    on = _grads_of(hip_device, cloud, cam, gc, None, use_depth=False)
    config.set_depth_gradient(False)
    off = _grads_of(hip_device, cloud, cam, gc, None, use_depth=False)
    for k in off:
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)


def test_switch_is_read_at_forward_time(hip_device, exact_mode):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    W, H = 128, 96
    cam, cloud = hp.box_setup(3_000, W, H, seed=7)
    camd = cam.to(hip_device)
    tfx, tfy = hp.tan_fov(cam)
    rs = GaussianRasterizationSettings(H, W, tfx, tfy, torch.zeros(3, device=hip_device), 1.0, camd.world_view_transform,
                                       camd.full_proj_transform, 0, camd.camera_center, False, False)
    gd = _upstream(H, W, 11).to(hip_device)

    def grad_with(fwd_on, bwd_on):
        m3 = cloud["means3D"].to(hip_device).clone().requires_grad_(True)
        config.set_depth_gradient(fwd_on)
        try:
            _, _, dep = GaussianRasterizer(rs)(means3D=m3, means2D=torch.zeros_like(m3, requires_grad=True),
                                               opacities=cloud["opacities"].to(hip_device), shs=cloud["shs"].to(hip_device),
                                               scales=cloud["scales"].to(hip_device), rotations=cloud["rotations"].to(hip_device))
            config.set_depth_gradient(bwd_on)
            (dep * gd).sum().backward()
        finally:
            config.set_depth_gradient(False)
        return m3.grad
    assert float(grad_with(False, True).abs().max()) == 0.0
    on = grad_with(True, True)
    assert float(on.abs().max()) > 0.0
    assert torch.equal(grad_with(True, False), on)


def test_depth_mode_is_bit_repeatable(hip_device, depth_on, exact_mode):
    W, H = 256, 192
    cam, cloud = hp.box_setup(20_000, W, H, seed=8, scale_mult=1.5)
    gc, gd = synthetic.upstream_grad(H, W), _upstream(H, W, 12)
    a = _grads_of(hip_device, cloud, cam, gc, gd)
    b = _grads_of(hip_device, cloud, cam, gc, gd)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_armed_fused_step_takes_the_depth_gradient(hip_device, depth_on):
    """install(fuse_step=True)'s armed FusedAdam (the raw node's no-zero-fill backward + masked step) in depth mode: the same
    parameter bits as backward + step() for a colour + depth loss."""
    from tests.test_gpu_optim import _adam_for, _two_clouds
    from luciddreamer_amd.gaussian_renderer import render_raw
    W, H = 320, 192
    a, b = _two_clouds(40_000, hip_device)
    names = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    for cl in (a, b):
        for n in names:
            setattr(cl, n, nn.Parameter(getattr(cl, n).detach()))
    opt_a, opt_b = _adam_for(a), _adam_for(b)
    cams = [c.to(hip_device) for c in cameras.rotate360_path(W, H, n_views=12)]
    bg = torch.zeros(3, device=hip_device)
    gen = torch.Generator().manual_seed(13)
    for it in range(4):
        cam = cams[(5 * it) % 12]
        g = torch.randn(3, H, W, generator=gen).to(hip_device)
        gd = torch.randn(1, H, W, generator=gen).to(hip_device)
        pa = render_raw(cam, a, bg_color=bg)
        ((pa["render"] * g).sum() + (pa["depth"] * gd).sum()).backward()
        opt_a.step()
        opt_a.zero_grad(set_to_none=True)
        assert opt_b.arm_fused_backward()
        pb = render_raw(cam, b, bg_color=bg)
        ((pb["render"] * g).sum() + (pb["depth"] * gd).sum()).backward()
        assert all(getattr(b, n).grad is None for n in names)
        opt_b.step()
        opt_b.zero_grad(set_to_none=True)
        assert torch.equal(pa["viewspace_points"].grad, pb["viewspace_points"].grad), it
        for n in names:
            assert torch.equal(getattr(a, n), getattr(b, n)), (it, n)


def test_c3_size_is_linear_and_finite(hip_device, depth_on):
    """C3 (1 M Gaussians, 1080p, beyond the Python oracle): grad(colour + depth) = grad(colour) + grad(depth) to float
    tolerance, nothing NaN or Inf."""
    from luciddreamer_amd.gaussian_renderer import GaussianCloud, render
    W, H = 1920, 1080
    c = synthetic.make_cloud(1_000_000, "band", 0)
    cam = cameras.rotate360_path(W, H, n_views=30)[3].to(hip_device)
    gc, gd = synthetic.upstream_grad(H, W).to(hip_device), _upstream(H, W, 14).to(hip_device)
    pc = GaussianCloud(c["means3D"].to(hip_device), c["scales"].to(hip_device), c["rotations"].to(hip_device),
                       c["opacities"].to(hip_device), c["shs"].to(hip_device), active_sh_degree=3)
    params = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")

    def grads(wc, wd):
        for n in params:
            getattr(pc, n).grad = None
        out = render(cam, pc)
        loss = (out["render"] * gc).sum() * wc + (out["depth"] * gd).sum() * wd
        loss.backward()
        return {"viewspace": out["viewspace_points"].grad.clone(), **{n: getattr(pc, n).grad.clone() for n in params}}
    both, col, dep = grads(1.0, 1.0), grads(1.0, 0.0), grads(0.0, 1.0)
    assert float(dep["_xyz"].abs().max()) > 0.0
    for k in both:
        assert bool(torch.isfinite(both[k]).all()) and bool(torch.isfinite(dep[k]).all()), k
        scale = float(both[k].abs().max())
        err = float((both[k] - (col[k] + dep[k])).abs().max())
        assert err <= 1e-4 * scale + 1e-30, (k, err, scale)


@pytest.mark.parametrize("path", ["compiled", "debug", "raw"])
@pytest.mark.parametrize("use_depth", [True, False], ids=["depth_in_loss", "depth_unused"])
def test_depth_mode_frees_its_nodes(hip_device, depth_on, exact_mode, path, use_depth):
    """With the switch on, a node keeps the forward's depth image for its backward.  Kept as the output itself, it would hold
    the node through its grad_fn (a cycle: nothing collects it in the compiled node, only the cyclic GC in the Python ones),
    and with the node its scratch buffers.  Iterations of forward + backward, outputs dropped, the cyclic GC off: the memory
    allocated on the device does not grow."""
    import gc
    from luciddreamer_amd.gaussian_renderer import GaussianCloud, render, render_raw
    W, H = 256, 192
    c = synthetic.make_cloud(20_000, "band", 5)
    cam = cameras.rotate360_path(W, H, n_views=12)[1].to(hip_device)
    pc = GaussianCloud(c["means3D"].to(hip_device), c["scales"].to(hip_device), c["rotations"].to(hip_device),
                       c["opacities"].to(hip_device), c["shs"].to(hip_device), active_sh_degree=1)
    gc_img, gd = synthetic.upstream_grad(H, W).to(hip_device), _upstream(H, W, 15).to(hip_device)
    opt = SimpleNamespace(debug=path == "debug", compute_cov3D_python=False, convert_SHs_python=False)
    fn = render_raw if path == "raw" else render

    def step():
        out = fn(cam, pc, opt)
        loss = (out["render"] * gc_img).sum() + ((out["depth"] * gd).sum() if use_depth else 0.0)
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
    assert grown < 256 * 1024, grown          # one leaked node alone holds its depth image (192 KB) and the scratch buffers
