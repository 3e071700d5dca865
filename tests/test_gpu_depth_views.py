"""Depth supervision in the multi-view step on the GPU: the masked depth L1 kernels (lr_depth_l1_*), ViewBatch with
grad_depths (lr_views_accumulate with dL_ddepth) and with depth_targets (the same call with targets), ViewStreams.run_view with
grad_depth on its fused, direct and engine paths and through the re-run of an overflowed view, and a C3-size step."""
import numpy as np
import pytest
import torch

from luciddreamer_amd import cameras, config, synthetic
from tests import depth_l1_ref, helpers as hp

pytestmark = pytest.mark.gpu

KEYS = {"means3D": "means3D", "means2D": "means2D", "opacity": "opacities", "sh": "shs", "scales": "scales",
        "rotations": "rotations"}


@pytest.fixture
def depth_on():
    config.set_depth_gradient(True)
    yield
    config.set_depth_gradient(False)


def _close(got, want, tol=2e-5, what=""):
    a, b = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    scale = np.abs(b).max()
    assert scale > 0, what
    err = np.abs(a - b).max()
    assert np.isfinite(a).all() and err <= tol * scale, (what, err, scale)


# ---- 1. the depth L1 kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 16), (257, 511), (512, 512), (1080, 1920)])
def test_depth_l1_kernel_matches_torch(hip_device, H, W):
    from luciddreamer_amd.loss import depth_l1
    depth, target = depth_l1_ref.make_pair(H, W, seed=H + W, lead=(1,))
    want, _ = depth_l1_ref.numpy_depth_l1(depth.numpy(), target.numpy(), 0.7)
    d = depth.to(hip_device).requires_grad_(True)
    t = target.to(hip_device)
    vals = []
    for _ in range(5):
        vals.append(depth_l1(d, t, 0.7).detach())
    got = float(vals[0])
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert all(torch.equal(v, vals[0]) for v in vals)                      # bit-repeatable: fixed-order reduction, no atomics
    (depth_l1(d, t, 0.7) * 1.3).backward()
    # torch autograd of the definition, float32, on the device: (1.3 * 0.7) / (H W) * sign * mask -- the same operations in the
    # same order, so the gradient is asserted bit for bit
    d_ref = depth.to(hip_device).requires_grad_(True)
    (depth_l1_ref.torch_depth_l1(d_ref, t, 0.7) * 1.3).backward()
    assert torch.equal(d.grad, d_ref.grad), float((d.grad - d_ref.grad).abs().max())
    assert float(d.grad.abs().max()) > 0
    # [H, W] inputs work the same
    d2 = depth[0].to(hip_device).requires_grad_(True)
    assert torch.equal(depth_l1(d2, t[0], 0.7).detach(), vals[0])


def test_depth_l1_all_masked_is_zero(hip_device):
    from luciddreamer_amd.loss import depth_l1
    for H, W in ((16, 16), (257, 511)):
        d = (1.0 + torch.rand(1, H, W)).to(hip_device).requires_grad_(True)
        t = torch.where(torch.rand(1, H, W) < 0.5, torch.zeros(1, H, W), torch.full((1, H, W), float("nan"))).to(hip_device)
        loss = depth_l1(d, t)
        loss.backward()
        assert float(loss.detach()) == 0.0 and not bool(d.grad.any())


# ---- 2./3. ViewBatch(grad_colors, grad_depths) -----------------------------------------------------------------------------
def _setup(hip_device, P, W, H, n_views, seed=6):
    cloud = synthetic.make_cloud(P, "band", seed)
    cams = [c.to(hip_device) for c in cameras.rotate360_path(W, H, n_views=n_views)]
    return cloud, cams


def _raster(c, W, H, bg, degree=3):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    tfx, tfy = hp.tan_fov(c)
    return GaussianRasterizer(GaussianRasterizationSettings(H, W, tfx, tfy, bg, 1.0, c.world_view_transform,
                                                            c.full_proj_transform, degree, c.camera_center, False, False))


def _acc_like(leaf, P):
    return {"means3D": torch.zeros_like(leaf["means3D"]), "means2D": torch.zeros(P, 3, device=leaf["means3D"].device),
            "opacity": torch.zeros_like(leaf["opacities"]), "sh": torch.zeros_like(leaf["shs"]),
            "scales": torch.zeros_like(leaf["scales"]), "rotations": torch.zeros_like(leaf["rotations"])}


def _run_batch(batch, leaf, acc):
    with torch.no_grad():
        batch.run(leaf["means3D"].detach(), leaf["opacities"].detach(), leaf["scales"].detach(), leaf["rotations"].detach(),
                  leaf["shs"].detach(), acc)


def test_view_batch_with_depth_equals_autograd_accumulation(hip_device, depth_on):
    from luciddreamer_amd import parallel
    P, W, H = 25_000, 256, 160
    cloud, cams = _setup(hip_device, P, W, H, 7)
    g = synthetic.upstream_grad(H, W).to(hip_device)
    gds = [torch.randn(1, H, W, generator=torch.Generator().manual_seed(20 + i)).to(hip_device) for i in range(len(cams))]
    bg = torch.tensor([0.1, 0.0, 0.2], device=hip_device)
    leaf = {k: v.to(hip_device).requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros(P, 3, device=hip_device, requires_grad=True)
    ref_depths = []
    for c, gd in zip(cams, gds):
        col, _, dep = _raster(c, W, H, bg)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"], shs=leaf["shs"],
                                           scales=leaf["scales"], rotations=leaf["rotations"])
        ((col * g).sum() + (dep * gd).sum()).backward()
        ref_depths.append(dep.detach().clone())
    ref = {k: v.grad.clone() for k, v in leaf.items()}
    ref["means2D"] = m2d.grad.clone()

    acc = _acc_like(leaf, P)
    depths = [torch.zeros(1, H, W, device=hip_device) for _ in cams]
    batch = parallel.ViewBatch(cams, [g] * len(cams), 3, bg, binning_capacity=400_000, n_streams=2, grad_depths=gds,
                               depths=depths)
    for _ in range(2):                               # run twice: workspace / streams / events are re-used
        for t in acc.values():
            t.zero_()
        _run_batch(batch, leaf, acc)
    batch.check()
    for k, rk in KEYS.items():
        _close(acc[k], ref[rk], what=k)
    for a, b in zip(depths, ref_depths):
        _close(a, b, tol=1e-5, what="depth")
    # the depth share is really there: colour-only differs
    acc0 = _acc_like(leaf, P)
    _run_batch(parallel.ViewBatch(cams, [g] * len(cams), 3, bg, binning_capacity=400_000, n_streams=2), leaf, acc0)
    assert float((acc0["means3D"] - acc["means3D"]).abs().max()) > 1e-3 * float(acc["means3D"].abs().max())
    # too small a capacity is reported, never written out of bounds
    small = parallel.ViewBatch(cams, [g] * len(cams), 3, bg, binning_capacity=500, n_streams=2, grad_depths=gds)
    _run_batch(small, leaf, acc)
    with pytest.raises(RuntimeError, match="capacity"):
        small.check()


@pytest.mark.parametrize("n_views", [1, 5])
def test_view_batch_with_depth_same_bits_for_every_number_of_chains(hip_device, n_views):
    from luciddreamer_amd import _lib, parallel
    P, W, H = 25_000, 256, 160
    cloud, cams = _setup(hip_device, P, W, H, 7)
    cams = cams[:n_views]
    cloud = {k: v.to(hip_device) for k, v in cloud.items()}
    g = synthetic.upstream_grad(H, W).to(hip_device)
    gds = [torch.randn(1, H, W, generator=torch.Generator().manual_seed(40 + i)).to(hip_device) for i in range(n_views)]
    bg = torch.tensor([0.1, 0.0, 0.2], device=hip_device)
    shapes = {"means3D": (P, 3), "means2D": (P, 3), "opacity": (P, 1), "sh": (P, 16, 3), "scales": (P, 3), "rotations": (P, 4)}
    _lib.tune_set("blend_quad", 2)
    _lib.tune_set("fwd_pair", 2)
    try:
        want = None
        for n_streams in (1, 2, 3, 4):
            batch = parallel.ViewBatch(cams, [g] * n_views, 3, bg, binning_capacity=400_000, n_streams=n_streams, grad_depths=gds)
            for _ in range(2):
                acc = {k: torch.zeros(s, device=hip_device) for k, s in shapes.items()}
                batch.run(cloud["means3D"], cloud["opacities"], cloud["scales"], cloud["rotations"], cloud["shs"], acc)
                got = {k: v.clone() for k, v in acc.items()}
                batch.check()
                if want is None:
                    want = got
                    assert all(float(v.abs().sum()) > 0 for v in want.values())
                for k in shapes:
                    assert torch.equal(got[k], want[k]), (n_streams, k)
    finally:
        _lib.tune_set("blend_quad", -1)
        _lib.tune_set("fwd_pair", -1)


# ---- 4. the fused training step with depth ---------------------------------------------------------------------------------
def _depth_targets(hip_device, cams, W, H, seed):
    """Targets near the rendered depth range, a third of the pixels without a target (0 or NaN)."""
    out = []
    for i, _ in enumerate(cams):
        gen = torch.Generator().manual_seed(seed + i)
        t = 2.0 + 6.0 * torch.rand(1, H, W, generator=gen)
        u = torch.rand(1, H, W, generator=gen)
        t = torch.where(u < 0.25, torch.zeros_like(t), t)
        t = torch.where((u >= 0.25) & (u < 0.33), torch.full_like(t, float("nan")), t)
        out.append(t.to(hip_device))
    return out


def test_view_batch_train_depth_equals_autograd(hip_device, depth_on):
    from luciddreamer_amd import parallel
    from luciddreamer_amd.loss import depth_l1, l1_dssim_loss
    P, W, H, w = 20_000, 256, 160, 0.35
    cloud, cams = _setup(hip_device, P, W, H, 5, seed=8)
    gen = torch.Generator().manual_seed(3)
    targets = [torch.rand(3, H, W, generator=gen).to(hip_device) for _ in cams]
    dts = _depth_targets(hip_device, cams, W, H, 70)
    bg = torch.tensor([0.0, 0.1, 0.0], device=hip_device)
    leaf = {k: v.to(hip_device).requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros(P, 3, device=hip_device, requires_grad=True)
    rows = []
    for c, tgt, dt in zip(cams, targets, dts):
        col, _, dep = _raster(c, W, H, bg)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"], shs=leaf["shs"],
                                           scales=leaf["scales"], rotations=leaf["rotations"])
        lc = l1_dssim_loss(col, tgt, 0.2)
        ld = depth_l1(dep, dt)
        (lc + w * ld).backward()
        rows.append([float(lc.detach()) + w * float(ld.detach()), float(ld.detach())])
    ref = {k: v.grad.clone() for k, v in leaf.items()}
    ref["means2D"] = m2d.grad.clone()

    acc = _acc_like(leaf, P)
    batch = parallel.ViewBatch(cams, None, 3, bg, binning_capacity=300_000, n_streams=3, targets=targets, lambda_dssim=0.2,
                               depth_targets=dts, depth_weight=w)
    _run_batch(batch, leaf, acc)
    batch.check()
    got = batch.losses.cpu().numpy()
    assert got.shape == (len(cams), 4)
    want = np.array(rows)
    assert np.abs(got[:, 0] - want[:, 0]).max() <= 1e-5 * np.abs(want[:, 0]).max()
    assert np.abs(got[:, 3] - want[:, 1]).max() <= 1e-5 * np.abs(want[:, 1]).max()
    assert np.all(want[:, 1] > 0)
    for k, rk in KEYS.items():
        _close(acc[k], ref[rk], what=k)


def test_view_batch_train_depth_weight_zero_is_the_colour_step(hip_device):
    from luciddreamer_amd import parallel
    P, W, H = 20_000, 256, 160
    cloud, cams = _setup(hip_device, P, W, H, 4, seed=9)
    leaf = {k: v.to(hip_device) for k, v in cloud.items()}
    gen = torch.Generator().manual_seed(4)
    targets = [torch.rand(3, H, W, generator=gen).to(hip_device) for _ in cams]
    dts = _depth_targets(hip_device, cams, W, H, 90)
    bg = torch.tensor([0.0, 0.1, 0.0], device=hip_device)
    colour = parallel.ViewBatch(cams, None, 3, bg, binning_capacity=300_000, n_streams=2, targets=targets)
    zero = parallel.ViewBatch(cams, None, 3, bg, binning_capacity=300_000, n_streams=2, targets=targets, depth_targets=dts,
                              depth_weight=0.0)
    a, b = _acc_like(leaf, P), _acc_like(leaf, P)
    _run_batch(colour, leaf, a)
    _run_batch(zero, leaf, b)
    colour.check()
    zero.check()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(colour.losses, zero.losses[:, :3])
    assert bool((zero.losses[:, 3] > 0).all())


# ---- 5. ViewStreams.run_view(grad_output=g, grad_depth=gd) -----------------------------------------------------------------
def _stream_step(hip_device, cloud, cams, W, H, g, gds, direct, starved=False, post=None):
    """One ViewStreams step over `cams` with fixed colour and depth gradients; returns (flat grads, means2D grad, recovered)."""
    from luciddreamer_amd import parallel
    P = cloud["means3D"].shape[0]
    bg = torch.zeros(3, device=hip_device)
    rast = [_raster(c, W, H, bg) for c in cams]
    leaf = {k: v.to(hip_device).requires_grad_(True) for k, v in cloud.items()}
    grads = parallel.FlatGrads(list(leaf.values()))
    m2d = torch.zeros(P, 3, device=hip_device, requires_grad=True)
    m2d.grad = torch.zeros_like(m2d)
    config.reset()
    config.set_async(True, headroom=1.0, warm_calls=1)
    config.set_fused_grad_accumulation(True)
    config.dropped_views = config.recovered_views = 0
    try:
        def fwd(r):
            col, _, dep = r(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"], shs=leaf["shs"],
                            scales=leaf["scales"], rotations=leaf["rotations"])
            return (col, dep) if post is None else post(col, dep)
        if starved:
            with torch.no_grad():
                fwd(rast[0])
            key = next(iter(config._hwm))
            config._hwm[key] = 64
        else:
            config.set_async(False)
        pipe = parallel.ViewStreams(hip_device, 2, direct=direct)
        pipe.begin_step()
        for r, gd in zip(rast, gds):
            pipe.run_view(lambda r=r: fwd(r), grad_output=g, grad_depth=gd)
        recovered = pipe.end_step()
        torch.cuda.synchronize()
    finally:
        config.set_fused_grad_accumulation(False)
        config.reset()
        config.set_async(True)
    return grads.flat.clone(), m2d.grad.clone(), recovered


def _autograd_sum(hip_device, cloud, cams, W, H, g, gds):
    from luciddreamer_amd import parallel
    P = cloud["means3D"].shape[0]
    bg = torch.zeros(3, device=hip_device)
    leaf = {k: v.to(hip_device).requires_grad_(True) for k, v in cloud.items()}
    grads = parallel.FlatGrads(list(leaf.values()))
    m2d = torch.zeros(P, 3, device=hip_device, requires_grad=True)
    config.set_async(False)
    try:
        for c, gd in zip(cams, gds):
            col, _, dep = _raster(c, W, H, bg)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"],
                                               shs=leaf["shs"], scales=leaf["scales"], rotations=leaf["rotations"])
            ((col * g).sum() + (dep * gd).sum()).backward()
    finally:
        config.set_async(True)
        config.reset()
    for v, p in zip(grads.views, leaf.values()):           # (in case autograd replaced a .grad instead of adding into it)
        if p.grad.data_ptr() != v.data_ptr():
            v.copy_(p.grad)
    return grads.flat.clone(), m2d.grad.clone()


@pytest.mark.parametrize("direct", [True, False], ids=["fused_path", "engine_path"])
def test_run_view_with_depth_equals_autograd(hip_device, depth_on, direct):
    P, W, H = 30_000, 320, 180
    cloud, cams = _setup(hip_device, P, W, H, 5, seed=4)
    g = synthetic.upstream_grad(H, W).to(hip_device)
    gds = [torch.randn(1, H, W, generator=torch.Generator().manual_seed(60 + i)).to(hip_device) for i in range(len(cams))]
    f_ref, m_ref = _autograd_sum(hip_device, cloud, cams, W, H, g, gds)
    f, m, _ = _stream_step(hip_device, cloud, cams, W, H, g, gds, direct)
    _close(f, f_ref, what="flat")
    _close(m, m_ref, what="means2D")
    f0, _ = _autograd_sum(hip_device, cloud, cams, W, H, g, [torch.zeros_like(gd) for gd in gds])
    assert float((f0 - f).abs().max()) > 1e-3 * float(f.abs().max())       # the depth share is in


@pytest.mark.parametrize("direct", [True, False], ids=["fused_path", "engine_path"])
def test_run_view_depth_refuses_what_it_cannot_honour(hip_device, direct):
    from luciddreamer_amd import parallel
    P, W, H = 5_000, 128, 96
    cloud, cams = _setup(hip_device, P, W, H, 2, seed=5)
    g = synthetic.upstream_grad(H, W).to(hip_device)
    gds = [torch.ones(1, H, W, device=hip_device)] * 2
    called = []
    pipe = parallel.ViewStreams(hip_device, 2, direct=direct)
    pipe.begin_step()
    with pytest.raises(ValueError, match="set_depth_gradient"):                # switch off: refused before forward_fn runs
        pipe.run_view(lambda: called.append(1), grad_output=g, grad_depth=gds[0])
    pipe.end_step()
    assert not called
    config.set_depth_gradient(True)
    try:
        for post in (lambda c, d: (c * 1.0, d), lambda c, d: (c, d.clamp(min=0.0)), lambda c, d: c):
            with pytest.raises(RuntimeError, match="rasterizer"):
                _stream_step(hip_device, cloud, cams, W, H, g, gds, direct, post=post)
    finally:
        config.set_depth_gradient(False)


@pytest.mark.parametrize("direct", [True, False], ids=["fused_path", "engine_path"])
def test_run_view_recovers_an_overflowed_view_with_its_depth_share(hip_device, depth_on, direct):
    P, W, H = 30_000, 320, 180
    cloud, cams = _setup(hip_device, P, W, H, 6, seed=4)
    g = synthetic.upstream_grad(H, W).to(hip_device)
    gds = [torch.randn(1, H, W, generator=torch.Generator().manual_seed(80 + i)).to(hip_device) for i in range(len(cams))]
    f_exact, m_exact, r0 = _stream_step(hip_device, cloud, cams, W, H, g, gds, direct)
    f_rec, m_rec, r1 = _stream_step(hip_device, cloud, cams, W, H, g, gds, direct, starved=True)
    assert r0 == 0 and r1 >= 1 and config.dropped_views == 0, (r0, r1, config.dropped_views)
    _close(f_rec, f_exact, tol=1e-5, what="flat")
    _close(m_rec, m_exact, tol=1e-5, what="means2D")


# ---- 6. C3 size -----------------------------------------------------------------------------------------------------------
def test_c3_size_views_accumulate_depth(hip_device, depth_on):
    """Three 1080p views of the 1 M cloud in ONE lr_views_accumulate call with dL_ddepth: finite, equal to the sum of three
    single-view depth-mode backward passes, and with zero depth gradients equal to the call without them."""
    from luciddreamer_amd import _C, parallel
    P, W, H = 1_000_000, 1920, 1080
    c = {k: v.to(hip_device) for k, v in synthetic.make_cloud(P, "band", 0).items()}
    cams = [cc.to(hip_device) for cc in cameras.rotate360_path(W, H, n_views=30)[2:5]]
    g = synthetic.upstream_grad(H, W).to(hip_device)
    gds = [torch.randn(1, H, W, generator=torch.Generator().manual_seed(100 + i)).to(hip_device) for i in range(3)]
    bg = torch.zeros(3, device=hip_device)
    leaf = {k: v.clone().requires_grad_(True) for k, v in c.items()}
    m2d = torch.zeros(P, 3, device=hip_device, requires_grad=True)
    config.set_async(False)
    n_rendered = []
    try:
        for cam, gd in zip(cams, gds):
            col, _, dep = _raster(cam, W, H, bg)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"],
                                                 shs=leaf["shs"], scales=leaf["scales"], rotations=leaf["rotations"])
            n_rendered.append(int(_C.last_num_rendered()))
            ((col * g).sum() + (dep * gd).sum()).backward()
    finally:
        config.set_async(True)
        config.reset()
    ref = {k: v.grad for k, v in leaf.items()}
    ref["means2D"] = m2d.grad
    cap = int(1.25 * max(n_rendered)) + 4096
    acc = _acc_like(leaf, P)
    batch = parallel.ViewBatch(cams, [g] * 3, 3, bg, binning_capacity=cap, n_streams=3, grad_depths=gds)
    _run_batch(batch, leaf, acc)
    batch.check()
    for k, rk in KEYS.items():
        assert bool(torch.isfinite(acc[k]).all()), k
        _close(acc[k], ref[rk], what=k)
    del ref, leaf, m2d
    zero = parallel.ViewBatch(cams, [g] * 3, 3, bg, binning_capacity=cap, n_streams=3,
                              grad_depths=[torch.zeros(1, H, W, device=hip_device)] * 3)
    plain = parallel.ViewBatch(cams, [g] * 3, 3, bg, binning_capacity=cap, n_streams=3)
    a, b = _acc_like(c, P), _acc_like(c, P)
    _run_batch(zero, c, a)
    _run_batch(plain, c, b)
    zero.check()
    plain.check()
    for k in KEYS:
        _close(a[k], b[k], what=k)
