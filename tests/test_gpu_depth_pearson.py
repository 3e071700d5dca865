"""The Pearson depth loss on the GPU: the kernels (lr_depth_pearson_*) against the float64 restatement of tests/depth_pearson_ref.py
-- ragged and multi-workgroup shapes, more partials than the final workgroup has threads, a near-constant depth map, the degenerate
inputs, invariance under a * t + b -- and the fused multi-view step with depth_loss="pearson" against the per-view composition
rasterizer -> l1_dssim_loss + w * depth_pearson -> backward, with masks, with densification statistics, with one degenerate view,
and with the defaults where they were.

The bars of the kernel tests: the arithmetic is double and is rounded to float once (6e-8), so 1e-6 on the value and 1e-6 of the
gradient's maximum leave a 16x margin."""
import numpy as np
import pytest
import torch

from luciddreamer_amd import cameras, config, synthetic
from tests import depth_pearson_ref as ref
from tests import helpers as hp
from tests.depth_l1_ref import numpy_depth_l1

pytestmark = pytest.mark.gpu

KEYS = {"means3D": "means3D", "means2D": "means2D", "opacity": "opacities", "sh": "shs", "scales": "scales",
        "rotations": "rotations"}


def _close(got, want, tol=2e-5, what=""):
    """The bar of tests/test_gpu_depth_views.py for the step against the autograd route."""
    a, b = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    scale = np.abs(b).max()
    assert scale > 0, what
    err = np.abs(a - b).max()
    assert np.isfinite(a).all() and err <= tol * scale, (what, err, scale)


def _assert_kernels_match(depth, target, dev, weight=0.7, upstream=1.3, what=""):
    """Value, rho and gradient of the device kernels against the float64 restatement on the same float32 arrays."""
    from luciddreamer_amd.loss import depth_correlation, depth_pearson
    want, rho, grad = ref.numpy_depth_pearson(depth.numpy(), target.numpy(), weight)
    d = depth.to(dev).requires_grad_(True)
    t = target.to(dev)
    loss = depth_pearson(d, t, weight)
    (loss * upstream).backward()
    got, got_rho = float(loss.detach()), float(depth_correlation(d, t))
    g = d.grad.cpu().numpy().astype(np.float64)
    scale = np.abs(grad).max()
    err = np.abs(g - upstream * grad).max()
    print(f"[depth pearson] {what} {tuple(depth.shape)}: loss {got:.8f} want {want:.8f} |diff| {abs(got - want):.2e}; rho {got_rho:.8f} "
          f"want {rho:.8f}; gradient max|g - g_ref| {err:.3e} of max|g_ref| {upstream * scale:.3e}")
    assert abs(got - want) <= 1e-6 and abs(got_rho - rho) <= 1e-6, (got, want, got_rho, rho)
    assert scale > 0 and np.isfinite(g).all() and err <= 1e-6 * upstream * scale, (err, scale)
    with np.errstate(invalid="ignore"):
        assert not g[~(target.numpy() > 0)].any()
    return d, t, loss.detach()


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------------
# (16,16) one ragged workgroup; (257,511) 65 workgroups with a ragged tail; (600,900) 264 workgroups: more partials than the
# final workgroup has threads, its loop over the partials runs twice
@pytest.mark.parametrize("H,W", [(16, 16), (257, 511), (600, 900)])
def test_kernels_match_the_float64_restatement(hip_device, H, W):
    from luciddreamer_amd.loss import depth_pearson
    depth, target = ref.make_pair(H, W, seed=H + W, lead=(1,))
    d, t, first = _assert_kernels_match(depth, target, hip_device, what="make_pair")
    vals = [depth_pearson(d, t, 0.7).detach() for _ in range(5)]
    assert all(torch.equal(v, first) for v in vals)                       # fixed-order double reduction, no atomics
    # [H, W] inputs: the same bits, value and gradient
    d2 = depth[0].to(hip_device).requires_grad_(True)
    l2 = depth_pearson(d2, t[0], 0.7)
    (l2 * 1.3).backward()
    assert torch.equal(l2.detach(), first) and tuple(d2.grad.shape) == (H, W) and torch.equal(d2.grad, d.grad[0])
    # the upstream scalar is honoured: 1.3 above (asserted against the restatement), and another one scales the same image
    d3 = depth.to(hip_device).requires_grad_(True)
    (depth_pearson(d3, t, 0.7) * -2.0).backward()
    want = ref.numpy_depth_pearson(depth.numpy(), target.numpy(), 0.7)[2] * -2.0
    assert np.abs(d3.grad.cpu().numpy() - want).max() <= 1e-6 * np.abs(want).max()


def test_near_constant_depth_keeps_its_variance(hip_device):
    """depth = 50 + 0.01 randn: sum d^2 is 3.3e8 and the centred sum 13, a cancellation of 7.4 digits.  With the five sums formed in
    float32 the restatement itself loses the variance altogether (Sxx comes out at -3e5 for 13: the input counts as degenerate, loss
    0 for 0.10529) -- a miss of 1.05e5 x the value's bar and 1e6 x the gradient's, confirmed below on the CPU before the device is
    asked."""
    H, W = 257, 511
    g = torch.Generator().manual_seed(11)
    depth = (50.0 + 0.01 * torch.randn(1, H, W, generator=g)).float()
    target = (depth + 0.005 * torch.randn(1, H, W, generator=g)).float()
    want, _, grad = ref.numpy_depth_pearson(depth.numpy(), target.numpy(), 0.7)
    f32, _, grad32 = ref.numpy_depth_pearson(depth.numpy(), target.numpy(), 0.7, accumulate=np.float32)
    assert 0.05 < want < 0.1
    assert abs(f32 - want) > 1e4 * 1e-6 and np.abs(grad32 - grad).max() > 1e4 * 1e-6 * np.abs(grad).max()
    _assert_kernels_match(depth, target, hip_device, what="near-constant")


def _degenerate_cases(H, W):
    g = torch.Generator().manual_seed(3)
    depth = 1.0 + torch.rand(1, H, W, generator=g)
    varied = 2.0 + torch.rand(1, H, W, generator=g)
    masked = torch.where(torch.rand(1, H, W, generator=g) < 0.5, torch.zeros(1, H, W), torch.full((1, H, W), float("nan")))
    one = masked.clone()
    one[0, H // 2, W // 3] = 2.5
    holes = torch.where(torch.rand(1, H, W, generator=g) < 0.3, torch.zeros(1, H, W), varied)
    return {"all_masked": (depth, masked), "one_valid_pixel": (depth, one),
            "constant_depth_on_valid": (torch.where(holes > 0, torch.full_like(depth, 4.25), depth), holes),
            "constant_target": (depth, torch.where(holes > 0, torch.full_like(holes, 3.5), holes))}


@pytest.mark.parametrize("case", ["all_masked", "one_valid_pixel", "constant_depth_on_valid", "constant_target"])
def test_degenerate_inputs_are_exactly_zero(hip_device, case):
    from luciddreamer_amd.loss import depth_correlation, depth_pearson
    for H, W in ((16, 16), (257, 511)):
        depth, target = _degenerate_cases(H, W)[case]
        assert ref.numpy_depth_pearson(depth.numpy(), target.numpy())[0] == 0.0
        d = depth.to(hip_device).requires_grad_(True)
        t = target.to(hip_device)
        loss = depth_pearson(d, t, 0.7)
        (loss * 1.3).backward()
        assert float(loss.detach()) == 0.0 and float(depth_correlation(d, t)) == 0.0
        assert not bool(d.grad.any()) and bool(torch.isfinite(d.grad).all())


@pytest.mark.parametrize("a,b", [(2.0, 0.0), (0.5, 3.0), (1.0, -0.3)])
def test_invariance_under_scale_and_shift_on_the_device(hip_device, a, b):
    """The transformed float32 target is another input (every pixel rounded anew), so the bar -- 1e-5 on the value, 1e-5 of the
    gradient's maximum -- is checked on the float64 restatement of the same transformed arrays first.  Valid targets are >= 0.5,
    so b = -0.3 moves no pixel out of the valid set.
    The pair is a GOOD estimate, depth + 0.1 randn with make_pair's pattern of missing targets: the residual must not dwarf the
    shift for the L1 comparison at the end to say anything (against make_pair's own unit-variance noise a shift of 0.3 moves the
    mean absolute residual by E|N(0.3, 1)| / E|N(0, 1)| - 1 = 4.5 % only; against 0.1 it triples it)."""
    from luciddreamer_amd.loss import depth_l1, depth_pearson
    H, W = 257, 511
    depth, pattern = ref.make_pair(H, W, seed=77, lead=(1,))
    target = torch.where(pattern > 0, depth + 0.1 * torch.randn(1, H, W, generator=torch.Generator().manual_seed(78)), pattern)
    target = torch.where((target > 0) & (target < 0.5), torch.zeros_like(target), target)
    moved = torch.where(target > 0, a * target + b, target)
    assert torch.equal(moved > 0, target > 0) and float(target[target > 0].min()) >= 0.5
    w0, _, g0 = ref.numpy_depth_pearson(depth.numpy(), target.numpy())
    w1, _, g1 = ref.numpy_depth_pearson(depth.numpy(), moved.numpy())
    assert abs(w1 - w0) <= 1e-5 and np.abs(g1 - g0).max() <= 1e-5 * np.abs(g0).max()
    out = []
    for tt in (target, moved):
        d = depth.to(hip_device).requires_grad_(True)
        loss = depth_pearson(d, tt.to(hip_device))
        loss.backward()
        out.append((float(loss.detach()), d.grad.cpu().numpy()))
    assert abs(out[1][0] - out[0][0]) <= 1e-5, (out[0][0], out[1][0])
    assert np.abs(out[1][1] - out[0][1]).max() <= 1e-5 * np.abs(out[0][1]).max()
    # the L1 term on the same pairs is another loss altogether
    l0 = float(depth_l1(depth.to(hip_device), target.to(hip_device)))
    l1 = float(depth_l1(depth.to(hip_device), moved.to(hip_device)))
    assert l0 == pytest.approx(numpy_depth_l1(depth.numpy(), target.numpy())[0], rel=1e-5)
    assert abs(l1 - l0) > 0.1 * l0, (l0, l1)


# ---- 2. the fused step against the per-view composition ---------------------------------------------------------------------
P, W, H, N_VIEWS, WD, WA = 25_000, 256, 160, 7, 0.35, 0.6


def _raster(c, bg, degree=3):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    tfx, tfy = hp.tan_fov(c)
    return GaussianRasterizer(GaussianRasterizationSettings(H, W, tfx, tfy, bg, 1.0, c.world_view_transform,
                                                            c.full_proj_transform, degree, c.camera_center, False, False))


def _render(c, bg, leaf, m2d, **kw):
    return _raster(c, bg)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"], shs=leaf["shs"],
                          scales=leaf["scales"], rotations=leaf["rotations"], **kw)


def _acc_like(leaf):
    dev = leaf["means3D"].device
    return {"means3D": torch.zeros(P, 3, device=dev), "means2D": torch.zeros(P, 3, device=dev), "opacity": torch.zeros(P, 1, device=dev),
            "sh": torch.zeros_like(leaf["shs"]), "scales": torch.zeros(P, 3, device=dev), "rotations": torch.zeros(P, 4, device=dev)}


def _run_batch(batch, leaf, acc, stats=None):
    with torch.no_grad():
        batch.run(leaf["means3D"], leaf["opacities"], leaf["scales"], leaf["rotations"], leaf["shs"], acc, stats=stats)


@pytest.fixture(scope="module")
def scene(hip_device):
    """25 000 Gaussians ("band"), 7 views of 256x160; colour targets, content masks, and depth targets an estimate would give: the
    scene's own rendered depth under a per-view scale and shift, with noise, a quarter of the pixels without a target (0 or NaN).
    The per-view compositions are computed once per variant and shared (S["ref"])."""
    from tests import mask_loss_ref
    from luciddreamer_amd.loss import content_mask
    dev = hip_device
    cloud = {k: v.to(dev) for k, v in synthetic.make_cloud(P, "band", 6).items()}
    cams = [c.to(dev) for c in cameras.rotate360_path(W, H, n_views=N_VIEWS)]
    bg = torch.tensor([0.1, 0.0, 0.2], device=dev)
    gen = torch.Generator().manual_seed(3)
    targets, masks, dts = [], [], []
    for i, c in enumerate(cams):
        with torch.no_grad():
            _, _, dep = _render(c, bg, cloud, torch.zeros(P, 3, device=dev))
        m = mask_loss_ref.make_mask(H, W, seed=100 + i)
        targets.append(((0.05 + torch.rand(3, H, W, generator=gen)) * m).to(dev))
        masks.append(content_mask(targets[-1]))
        a, b = 0.5 + 1.5 * float(torch.rand(1, generator=gen)), float(torch.rand(1, generator=gen))
        t = a * dep.cpu().reshape(1, H, W) + b + 0.3 * torch.randn(1, H, W, generator=gen).abs()
        u = torch.rand(1, H, W, generator=gen)
        t = torch.where(u < 0.2, torch.zeros_like(t), t)
        t = torch.where((u >= 0.2) & (u < 0.25), torch.full_like(t, float("nan")), t)
        dts.append(t.to(dev))
    return {"cloud": cloud, "cams": cams, "bg": bg, "targets": targets, "masks": masks, "dts": dts, "ref": {}}


def _composition(S, with_masks=False, no_depth_views=(), dts=None):
    """Per view: rasterizer -> colour loss + WD * depth_pearson [+ WA * alpha_hole] -> backward, summed over the views; with the
    densification statistics the per-view route leaves (norm of each view's own screen-space gradient, visits, radii)."""
    from luciddreamer_amd.loss import alpha_hole, depth_correlation, depth_pearson, l1_dssim_loss, masked_l1_dssim
    key = (with_masks, tuple(no_depth_views), dts is None)
    if key in S["ref"]:
        return S["ref"][key]
    dev = S["bg"].device
    dts = S["dts"] if dts is None else dts
    leaf = {k: v.clone().requires_grad_(True) for k, v in S["cloud"].items()}
    m2d_sum = torch.zeros(P, 3, device=dev)
    stat_a, stat_d, stat_r = torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    rows = []
    config.set_depth_gradient(True)
    try:
        for i, c in enumerate(S["cams"]):
            m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
            if with_masks:
                col, radii, dep, alp = _render(c, S["bg"], leaf, m2d, return_alpha=True)
                loss = masked_l1_dssim(col, S["targets"][i], S["masks"][i], 0.2) + WA * alpha_hole(alp, S["masks"][i])
            else:
                col, radii, dep = _render(c, S["bg"], leaf, m2d)
                loss = l1_dssim_loss(col, S["targets"][i], 0.2)
            rho = float(depth_correlation(dep, dts[i]))
            if i not in no_depth_views:
                loss = loss + WD * depth_pearson(dep, dts[i])
            loss.backward()
            rows.append([float(loss.detach()), rho])
            vis = radii > 0
            m2d_sum += m2d.grad
            stat_a += torch.where(vis, m2d.grad[:, :2].norm(dim=1), torch.zeros_like(stat_a))
            stat_d += vis.float()
            stat_r = torch.maximum(stat_r, radii.clamp(min=0).float())
    finally:
        config.set_depth_gradient(False)
    grads = {k: v.grad.clone() for k, v in leaf.items()}
    grads["means2D"] = m2d_sum
    S["ref"][key] = {"grads": grads, "rows": np.array(rows), "stats": (stat_a, stat_d, stat_r)}
    return S["ref"][key]


def _pearson_batch(S, depth_weight=WD, **kw):
    from luciddreamer_amd import parallel
    kw.setdefault("depth_targets", S["dts"])
    return parallel.ViewBatch(S["cams"], None, 3, S["bg"], binning_capacity=400_000, n_streams=2, targets=S["targets"],
                              lambda_dssim=0.2, depth_weight=depth_weight, depth_loss="pearson", **kw)


@pytest.mark.parametrize("with_masks", [False, True], ids=["depth", "mask_depth"])
def test_fused_step_equals_the_per_view_composition(hip_device, scene, with_masks):
    want = _composition(scene, with_masks)
    rho = want["rows"][:, 1]
    assert np.all(rho > 0.3) and np.all(1.0 - rho > 1e-4), rho             # correlated targets, not a trivial term
    batch = _pearson_batch(scene, **(dict(masks=scene["masks"], alpha_weight=WA) if with_masks else {}))
    acc = _acc_like(scene["cloud"])
    for _ in range(2):                                                     # run twice: workspace, streams and events are re-used
        for t in acc.values():
            t.zero_()
        _run_batch(batch, scene["cloud"], acc)
    batch.check()
    got = batch.losses.cpu().numpy()
    assert got.shape == (N_VIEWS, 5 if with_masks else 4)
    print(f"[depth pearson step] 1 - rho per view: step {got[:, 3]}, composition {1.0 - rho}")
    assert np.abs(got[:, 3] - (1.0 - rho)).max() <= 1e-5 * np.abs(1.0 - rho).max()
    assert np.abs(got[:, 0] - want["rows"][:, 0]).max() <= 1e-5 * np.abs(want["rows"][:, 0]).max()
    for k, rk in KEYS.items():
        _close(acc[k], want["grads"][rk], what=k)
    # the depth share is really there: the colour-only gradients of the same step differ
    zero = _pearson_batch(scene, depth_weight=0.0, **(dict(masks=scene["masks"], alpha_weight=WA) if with_masks else {}))
    acc0 = _acc_like(scene["cloud"])
    _run_batch(zero, scene["cloud"], acc0)
    assert float((acc0["means3D"] - acc["means3D"]).abs().max()) > 1e-3 * float(acc["means3D"].abs().max())


def test_fused_step_statistics_equal_the_per_view_route(hip_device, scene):
    """densify_stats="grad" composes unchanged: visits and radii exact, the norm sum within the project's bar for the screen-space
    gradient (tests/test_gpu_views_stats.py), and the step's gradients keep their bits."""
    want = _composition(scene)
    stat_a, stat_d, stat_r = want["stats"]
    dev = hip_device
    stats = {"xyz_gradient_accum": torch.zeros(P, 1, device=dev), "denom": torch.zeros(P, 1, device=dev),
             "max_radii2D": torch.zeros(P, device=dev)}
    acc, plain = _acc_like(scene["cloud"]), _acc_like(scene["cloud"])
    batch = _pearson_batch(scene, densify_stats="grad")
    _run_batch(batch, scene["cloud"], acc, stats)
    batch.check()
    _run_batch(_pearson_batch(scene), scene["cloud"], plain)
    for k in acc:
        assert torch.equal(acc[k], plain[k]), k
    assert torch.equal(stats["denom"][:, 0], stat_d) and torch.equal(stats["max_radii2D"], stat_r)
    assert float(stat_d.max()) > 1 and float(stat_a.max()) > 0
    hp.compare_grads({"accum": stats["xyz_gradient_accum"].double().cpu().numpy().reshape(-1)},
                     {"accum": stat_a.double().cpu().numpy()}, names=["accum"])


def test_defaults_did_not_move(hip_device, scene):
    from luciddreamer_amd import parallel
    S = scene
    common = dict(binning_capacity=400_000, n_streams=2, targets=S["targets"], lambda_dssim=0.2)

    def run(**kw):
        b = parallel.ViewBatch(S["cams"], None, 3, S["bg"], **common, **kw)
        acc = _acc_like(S["cloud"])
        _run_batch(b, S["cloud"], acc)
        b.check()
        return acc, b.losses.clone()
    # depth_loss="l1" is the step without the argument, bit for bit
    a, la = run(depth_targets=S["dts"], depth_weight=WD)
    b, lb = run(depth_targets=S["dts"], depth_weight=WD, depth_loss="l1")
    assert all(torch.equal(a[k], b[k]) for k in a) and torch.equal(la, lb)
    assert float(a["means3D"].abs().max()) > 0
    # depth_weight 0 in Pearson mode: the colour-only step's accumulators bit for bit, the term still reported
    c, lc = run()
    z, lz = run(depth_targets=S["dts"], depth_weight=0.0, depth_loss="pearson")
    assert all(torch.equal(c[k], z[k]) for k in c) and torch.equal(lc, lz[:, :3])
    rho = _composition(S)["rows"][:, 1]
    assert np.abs(lz[:, 3].cpu().numpy() - (1.0 - rho)).max() <= 1e-5 * np.abs(1.0 - rho).max()


def test_one_degenerate_view_inside_a_step(hip_device, scene):
    """View 2 has no depth target at all: its term is 0, its gradients the colour-only ones, and nothing is non-finite."""
    S = scene
    dts = list(S["dts"])
    dts[2] = torch.zeros_like(dts[2])
    want = _composition(S, no_depth_views=(2,), dts=dts)
    assert want["rows"][2, 1] == 0.0
    batch = _pearson_batch(S, depth_targets=dts)
    acc = _acc_like(S["cloud"])
    _run_batch(batch, S["cloud"], acc)
    batch.check()
    got = batch.losses.cpu().numpy()
    assert np.isfinite(got).all() and got[2, 3] == 0.0 and np.all(np.delete(got[:, 3], 2) > 0)
    assert np.abs(got[:, 0] - want["rows"][:, 0]).max() <= 1e-5 * np.abs(want["rows"][:, 0]).max()
    for k, rk in KEYS.items():
        assert bool(torch.isfinite(acc[k]).all()), k
        _close(acc[k], want["grads"][rk], what=k)
