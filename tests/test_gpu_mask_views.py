"""Mask supervision in the multi-view step on the GPU: the masked L1 + DSSIM kernels (lr_masked_l1_dssim_*) against the float64
oracle and, for an all-ones mask, against lr_l1_dssim_* bit for bit; the alpha hole term (lr_alpha_hole_*); ViewBatch with
grad_alphas (lr_views_accumulate with dL_dalpha) and with masks (the same call with masks) against the autograd route, the same bits
for every number of chains, and a C3-size step."""
import numpy as np
import pytest
import torch

from luciddreamer_amd import cameras, config, synthetic
from tests import helpers as hp
from tests import mask_loss_ref

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


# ---- 1. the masked L1 + DSSIM kernels ---------------------------------------------------------------------------------------
def _masked_run(img, gt, m, dev, upstream=2.5):
    from luciddreamer_amd.loss import masked_l1_dssim
    x = torch.tensor(img, device=dev, requires_grad=True)
    loss = masked_l1_dssim(x, torch.tensor(gt, device=dev), torch.tensor(m, device=dev), 0.2)
    (loss * upstream).backward()
    return float(loss.item()), x.grad.cpu().numpy()


@pytest.mark.parametrize("shape", [(3, 97, 131), (3, 256, 256), (3, 512, 512), (3, 1080, 1920)])
@pytest.mark.parametrize("kind", ["soft", "binary"])
def test_masked_l1_dssim_matches_oracle(hip_device, shape, kind):
    C, H, W = shape
    rng = np.random.default_rng(H + W)
    gt = rng.random(shape).astype(np.float32)
    img = np.clip(0.6 * gt + 0.4 * rng.random(shape), 0, 1).astype(np.float32)
    m = mask_loss_ref.make_mask(H, W, seed=H * 3 + W, kind=kind).numpy()
    loss, grad = _masked_run(img, gt, m, hip_device)
    assert np.isfinite(grad).all()
    assert not grad[:, m[0] == 0].any()                                   # nothing reaches a hole
    if H * W > 1_000_000:
        # the oracle's loss on the whole image, its gradient through cropped runs (as tests/test_gpu_loss.py)
        o = mask_loss_ref.numpy_masked_l1_dssim(img, gt, m, 0.2, want_grad=False)
        assert abs(loss - o["loss"]) <= 2e-6
        n_full = C * H * W
        for (y0, x0) in ((0, 0), (H - 96, W - 96), (H // 2 - 48, W // 2 - 48), (0, W // 2)):
            crop = (slice(None), slice(y0, y0 + 96), slice(x0, x0 + 96))
            oc = mask_loss_ref.numpy_masked_l1_dssim(img[crop], gt[crop], m[crop], 0.2)
            ref = 2.5 * oc["grad"] * (C * 96 * 96) / n_full
            inner = np.ones((96, 96), bool)
            if y0 > 0: inner[:10] = False
            if y0 + 96 < H: inner[-10:] = False
            if x0 > 0: inner[:, :10] = False
            if x0 + 96 < W: inner[:, -10:] = False
            assert np.abs(grad[crop] - ref)[:, inner].max() <= 2e-5 * np.abs(ref).max()
        return
    o = mask_loss_ref.numpy_masked_l1_dssim(img, gt, m, 0.2)
    assert abs(loss - o["loss"]) <= 2e-6
    ref = 2.5 * o["grad"]
    assert np.abs(grad - ref).max() <= 2e-5 * np.abs(ref).max()


@pytest.mark.parametrize("shape", [(3, 97, 131), (3, 1080, 1920)])
def test_all_ones_mask_gives_the_plain_loss_bits(hip_device, shape):
    from luciddreamer_amd.loss import l1_dssim_loss, masked_l1_dssim
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(shape, generator=g).to(hip_device)
    x0 = torch.rand(shape, generator=g).to(hip_device)
    ones = torch.ones(1, *shape[1:], device=hip_device)
    a = x0.clone().requires_grad_(True)
    b = x0.clone().requires_grad_(True)
    la = l1_dssim_loss(a, gt, 0.2)
    lb = masked_l1_dssim(b, gt, ones, 0.2)
    (la * 1.7).backward()
    (lb * 1.7).backward()
    assert torch.equal(la.detach(), lb.detach())
    assert torch.equal(a.grad, b.grad)


# ---- 2. the alpha hole term --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 16), (257, 511), (512, 512), (1080, 1920)])
def test_alpha_hole_matches_torch(hip_device, H, W):
    from luciddreamer_amd.loss import alpha_hole
    g = torch.Generator().manual_seed(H + W)
    alpha = torch.rand(1, H, W, generator=g)
    m = mask_loss_ref.make_mask(H, W, seed=W, kind="binary" if H > 16 else "soft")
    want, _ = mask_loss_ref.numpy_alpha_hole(alpha.numpy(), m.numpy(), 0.7)
    a = alpha.to(hip_device).requires_grad_(True)
    md = m.to(hip_device)
    vals = [alpha_hole(a, md, 0.7).detach() for _ in range(5)]
    assert abs(float(vals[0]) - want) <= 1e-6 * abs(want), (float(vals[0]), want)
    assert all(torch.equal(v, vals[0]) for v in vals)                      # bit-repeatable
    (alpha_hole(a, md, 0.7) * 1.3).backward()
    a_ref = alpha.to(hip_device).requires_grad_(True)
    (mask_loss_ref.torch_alpha_hole(a_ref, md, 0.7) * 1.3).backward()
    assert torch.equal(a.grad, a_ref.grad), float((a.grad - a_ref.grad).abs().max())
    assert float(a.grad.abs().max()) > 0
    assert torch.equal(alpha_hole(a[0], md[0], 0.7).detach(), vals[0])     # [H, W] inputs work the same


# ---- 3. ViewBatch(grad_colors, grad_alphas=...) ------------------------------------------------------------------------------
def _setup(hip_device, P, W, H, n_views, seed=6):
    cloud = synthetic.make_cloud(P, "band", seed)
    cams = [c.to(hip_device) for c in cameras.rotate360_path(W, H, n_views=n_views)]
    return cloud, cams


def _raster(c, W, H, bg, degree=3):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    tfx, tfy = hp.tan_fov(c)
    return GaussianRasterizer(GaussianRasterizationSettings(H, W, tfx, tfy, bg, 1.0, c.world_view_transform,
                                                            c.full_proj_transform, degree, c.camera_center, False, False))


def _render(c, W, H, bg, leaf, m2d):
    return _raster(c, W, H, bg)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"], shs=leaf["shs"],
                                scales=leaf["scales"], rotations=leaf["rotations"], return_alpha=True)


def _acc_like(leaf, P):
    return {"means3D": torch.zeros_like(leaf["means3D"]), "means2D": torch.zeros(P, 3, device=leaf["means3D"].device),
            "opacity": torch.zeros_like(leaf["opacities"]), "sh": torch.zeros_like(leaf["shs"]),
            "scales": torch.zeros_like(leaf["scales"]), "rotations": torch.zeros_like(leaf["rotations"])}


def _run_batch(batch, leaf, acc):
    with torch.no_grad():
        batch.run(leaf["means3D"].detach(), leaf["opacities"].detach(), leaf["scales"].detach(), leaf["rotations"].detach(),
                  leaf["shs"].detach(), acc)


@pytest.mark.parametrize("with_depth", [False, True], ids=["alpha", "depth_alpha"])
def test_view_batch_with_alpha_equals_autograd_accumulation(hip_device, depth_on, with_depth):
    from luciddreamer_amd import parallel
    P, W, H = 25_000, 256, 160
    cloud, cams = _setup(hip_device, P, W, H, 7)
    g = synthetic.upstream_grad(H, W).to(hip_device)
    gas = [torch.randn(1, H, W, generator=torch.Generator().manual_seed(30 + i)).to(hip_device) for i in range(len(cams))]
    gds = [torch.randn(1, H, W, generator=torch.Generator().manual_seed(20 + i)).to(hip_device) for i in range(len(cams))] \
        if with_depth else None
    bg = torch.tensor([0.1, 0.0, 0.2], device=hip_device)
    leaf = {k: v.to(hip_device).requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros(P, 3, device=hip_device, requires_grad=True)
    ref_alphas = []
    for i, (c, ga) in enumerate(zip(cams, gas)):
        col, _, dep, alp = _render(c, W, H, bg, leaf, m2d)
        loss = (col * g).sum() + (alp * ga).sum()
        if with_depth:
            loss = loss + (dep * gds[i]).sum()
        loss.backward()
        ref_alphas.append(alp.detach().clone())
    ref = {k: v.grad.clone() for k, v in leaf.items()}
    ref["means2D"] = m2d.grad.clone()

    acc = _acc_like(leaf, P)
    alphas = [torch.zeros(1, H, W, device=hip_device) for _ in cams]
    batch = parallel.ViewBatch(cams, [g] * len(cams), 3, bg, binning_capacity=400_000, n_streams=2, grad_depths=gds,
                               grad_alphas=gas, alphas=alphas)
    for _ in range(2):                               # run twice: workspace / streams / events are re-used
        for t in acc.values():
            t.zero_()
        _run_batch(batch, leaf, acc)
    batch.check()
    for k, rk in KEYS.items():
        _close(acc[k], ref[rk], what=k)
    for a, b in zip(alphas, ref_alphas):
        _close(a, b, tol=1e-5, what="alpha")          # lr_render_alpha's values
    # the alpha share is really there
    acc0 = _acc_like(leaf, P)
    _run_batch(parallel.ViewBatch(cams, [g] * len(cams), 3, bg, binning_capacity=400_000, n_streams=2, grad_depths=gds), leaf,
               acc0)
    assert float((acc0["opacity"] - acc["opacity"]).abs().max()) > 1e-3 * float(acc["opacity"].abs().max())


# ---- 4. the fused training step with masks -----------------------------------------------------------------------------------
def _depth_targets(hip_device, cams, W, H, seed):
    out = []
    for i, _ in enumerate(cams):
        gen = torch.Generator().manual_seed(seed + i)
        t = 2.0 + 6.0 * torch.rand(1, H, W, generator=gen)
        t = torch.where(torch.rand(1, H, W, generator=gen) < 0.25, torch.zeros_like(t), t)
        out.append(t.to(hip_device))
    return out


def _holey_targets(hip_device, cams, W, H, seed):
    """Targets with LucidDreamer's holes (exact zeros) and the content masks rebuilt from them (loss.content_mask)."""
    from luciddreamer_amd.loss import content_mask
    targets, masks = [], []
    for i, _ in enumerate(cams):
        gen = torch.Generator().manual_seed(seed + i)
        m = mask_loss_ref.make_mask(H, W, seed=seed + 100 + i)
        t = (0.05 + torch.rand(3, H, W, generator=gen)) * m
        targets.append(t.to(hip_device))
        masks.append(content_mask(targets[-1]))
        assert torch.equal(masks[-1].cpu(), m)
    return targets, masks


@pytest.mark.parametrize("with_depth", [False, True], ids=["mask", "mask_depth"])
def test_view_batch_train_mask_equals_autograd_recipe(hip_device, depth_on, with_depth):
    from luciddreamer_amd import parallel
    from luciddreamer_amd.loss import alpha_hole, depth_l1, masked_l1_dssim
    P, W, H, wa, wd = 20_000, 256, 160, 0.6, 0.35
    cloud, cams = _setup(hip_device, P, W, H, 5, seed=8)
    targets, masks = _holey_targets(hip_device, cams, W, H, 3)
    dts = _depth_targets(hip_device, cams, W, H, 70) if with_depth else None
    bg = torch.tensor([0.0, 0.1, 0.0], device=hip_device)
    leaf = {k: v.to(hip_device).requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros(P, 3, device=hip_device, requires_grad=True)
    rows = []
    for i, (c, tgt, m) in enumerate(zip(cams, targets, masks)):
        col, _, dep, alp = _render(c, W, H, bg, leaf, m2d)
        # INTEGRATION.md 2e composed with torch ops: the masked pair's l1 and ssim, the hole term
        x, gm = col * m, tgt * m
        l1 = (x - gm).abs().mean()
        s = 1.0 - masked_l1_dssim(col, tgt, m, 1.0)                 # the masked pair's ssim (lambda 1: 1 - ssim)
        lc = masked_l1_dssim(col, tgt, m, 0.2)
        la = mask_loss_ref.torch_alpha_hole(alp, m)
        loss = lc + wa * la
        ld = depth_l1(dep, dts[i]) if with_depth else torch.zeros((), device=hip_device)
        if with_depth:
            loss = loss + wd * ld
        loss.backward()
        rows.append([float(loss.detach()), float(l1.detach()), float(s.detach()), float(ld.detach()), float(la.detach())])
    ref = {k: v.grad.clone() for k, v in leaf.items()}
    ref["means2D"] = m2d.grad.clone()

    acc = _acc_like(leaf, P)
    alphas = [torch.zeros(1, H, W, device=hip_device) for _ in cams]
    batch = parallel.ViewBatch(cams, None, 3, bg, binning_capacity=300_000, n_streams=3, targets=targets, lambda_dssim=0.2,
                               masks=masks, alpha_weight=wa, depth_targets=dts, depth_weight=wd if with_depth else None,
                               alphas=alphas)
    _run_batch(batch, leaf, acc)
    batch.check()
    got = batch.losses.cpu().numpy()
    assert got.shape == (len(cams), 5)
    want = np.array(rows)
    for j in range(5):
        scale = max(np.abs(want[:, j]).max(), 1e-6)
        assert np.abs(got[:, j] - want[:, j]).max() <= 1e-5 * scale, (j, got[:, j], want[:, j])
    assert np.all(want[:, 4] > 0)
    if not with_depth:
        assert not got[:, 3].any()
    for k, rk in KEYS.items():
        _close(acc[k], ref[rk], what=k)
    for c, a in zip(cams, alphas):
        with torch.no_grad():
            _close(a, _render(c, W, H, bg, leaf, torch.zeros(P, 3, device=hip_device))[3], tol=1e-5, what="alpha")
    # the alpha share is really there: weight 0 differs
    acc0 = _acc_like(leaf, P)
    _run_batch(parallel.ViewBatch(cams, None, 3, bg, binning_capacity=300_000, n_streams=3, targets=targets, masks=masks,
                                  alpha_weight=0.0, depth_targets=dts, depth_weight=wd if with_depth else None), leaf, acc0)
    assert float((acc0["opacity"] - acc["opacity"]).abs().max()) > 1e-3 * float(acc["opacity"].abs().max())


@pytest.mark.parametrize("with_depth", [False, True], ids=["colour", "depth"])
def test_view_batch_train_mask_weight_zero_all_ones_is_todays_step(hip_device, with_depth):
    from luciddreamer_amd import parallel
    P, W, H = 20_000, 256, 160
    cloud, cams = _setup(hip_device, P, W, H, 4, seed=9)
    leaf = {k: v.to(hip_device) for k, v in cloud.items()}
    gen = torch.Generator().manual_seed(4)
    targets = [torch.rand(3, H, W, generator=gen).to(hip_device) for _ in cams]
    ones = [torch.ones(1, H, W, device=hip_device) for _ in cams]
    dts = _depth_targets(hip_device, cams, W, H, 90) if with_depth else None
    dw = 0.4 if with_depth else None
    bg = torch.tensor([0.0, 0.1, 0.0], device=hip_device)
    today = parallel.ViewBatch(cams, None, 3, bg, binning_capacity=300_000, n_streams=2, targets=targets, depth_targets=dts,
                               depth_weight=dw)
    zero = parallel.ViewBatch(cams, None, 3, bg, binning_capacity=300_000, n_streams=2, targets=targets, depth_targets=dts,
                              depth_weight=dw, masks=ones, alpha_weight=0.0)
    a, b = _acc_like(leaf, P), _acc_like(leaf, P)
    _run_batch(today, leaf, a)
    _run_batch(zero, leaf, b)
    today.check()
    zero.check()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    n = 4 if with_depth else 3
    assert torch.equal(today.losses[:, :n], zero.losses[:, :n])
    assert not bool(zero.losses[:, 4].any())                  # all content: no hole term


@pytest.mark.parametrize("n_views", [1, 5])
def test_view_batch_with_masks_same_bits_for_every_number_of_chains(hip_device, n_views):
    from luciddreamer_amd import _lib, parallel
    P, W, H = 25_000, 256, 160
    cloud, cams = _setup(hip_device, P, W, H, 7)
    cams = cams[:n_views]
    cloud = {k: v.to(hip_device) for k, v in cloud.items()}
    g = synthetic.upstream_grad(H, W).to(hip_device)
    gas = [torch.randn(1, H, W, generator=torch.Generator().manual_seed(40 + i)).to(hip_device) for i in range(n_views)]
    targets, masks = _holey_targets(hip_device, cams, W, H, 50)
    bg = torch.tensor([0.1, 0.0, 0.2], device=hip_device)
    shapes = {"means3D": (P, 3), "means2D": (P, 3), "opacity": (P, 1), "sh": (P, 16, 3), "scales": (P, 3), "rotations": (P, 4)}
    _lib.tune_set("blend_quad", 2)
    _lib.tune_set("fwd_pair", 2)
    try:
        for make in (lambda n: parallel.ViewBatch(cams, [g] * n_views, 3, bg, binning_capacity=400_000, n_streams=n,
                                                  grad_alphas=gas),
                     lambda n: parallel.ViewBatch(cams, None, 3, bg, binning_capacity=400_000, n_streams=n, targets=targets,
                                                  masks=masks, alpha_weight=0.5)):
            want = want_l = None
            for n_streams in (1, 2, 3, 4):
                batch = make(n_streams)
                for _ in range(2):
                    acc = {k: torch.zeros(s, device=hip_device) for k, s in shapes.items()}
                    batch.run(cloud["means3D"], cloud["opacities"], cloud["scales"], cloud["rotations"], cloud["shs"], acc)
                    got = {k: v.clone() for k, v in acc.items()}
                    got_l = None if batch.losses is None else batch.losses.clone()
                    batch.check()
                    if want is None:
                        want, want_l = got, got_l
                        assert all(float(v.abs().sum()) > 0 for v in want.values())
                    for k in shapes:
                        assert torch.equal(got[k], want[k]), (n_streams, k)
                    if got_l is not None:
                        assert torch.equal(got_l, want_l), n_streams
    finally:
        _lib.tune_set("blend_quad", -1)
        _lib.tune_set("fwd_pair", -1)


# ---- 5. C3 size ---------------------------------------------------------------------------------------------------------------
def test_c3_size_views_train_mask(hip_device):
    """Three 1080p views of the 1 M cloud in ONE lr_views_accumulate call with masks: finite, and equal to the sum of three
    single-view calls."""
    from luciddreamer_amd import _C, parallel
    P, W, H = 1_000_000, 1920, 1080
    c = {k: v.to(hip_device) for k, v in synthetic.make_cloud(P, "band", 0).items()}
    cams = [cc.to(hip_device) for cc in cameras.rotate360_path(W, H, n_views=30)[2:5]]
    targets, masks = _holey_targets(hip_device, cams, W, H, 200)
    bg = torch.zeros(3, device=hip_device)
    config.set_async(False)
    n_rendered = []
    try:
        with torch.no_grad():
            for cam in cams:
                _raster(cam, W, H, bg)(means3D=c["means3D"], means2D=torch.zeros_like(c["means3D"]), opacities=c["opacities"],
                                       shs=c["shs"], scales=c["scales"], rotations=c["rotations"])
                n_rendered.append(int(_C.last_num_rendered()))
    finally:
        config.set_async(True)
        config.reset()
    cap = int(1.25 * max(n_rendered)) + 4096
    acc = _acc_like(c, P)
    batch = parallel.ViewBatch(cams, None, 3, bg, binning_capacity=cap, n_streams=3, targets=targets, masks=masks,
                               alpha_weight=0.5)
    _run_batch(batch, c, acc)
    batch.check()
    ref = _acc_like(c, P)
    rows = []
    for i in range(3):
        one = parallel.ViewBatch(cams[i:i + 1], None, 3, bg, binning_capacity=cap, n_streams=1, targets=targets[i:i + 1],
                                 masks=masks[i:i + 1], alpha_weight=0.5)
        _run_batch(one, c, ref)
        one.check()
        rows.append(one.losses.clone())
    _close(batch.losses, torch.cat(rows), tol=1e-5, what="losses")
    assert bool(torch.isfinite(batch.losses).all()) and bool((batch.losses[:, 4] > 0).all())
    for k in KEYS:
        assert bool(torch.isfinite(acc[k]).all()), k
        _close(acc[k], ref[k], what=k)
