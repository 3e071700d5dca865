"""Densification statistics inside the multi-view step on the GPU: ViewBatch(densify_stats="grad" | "absgrad") -> lr_views_accumulate
with the stat_* members, against the float64 per-pixel reference (tests/absgrad_ref.py), against the per-view route on the same
device (forward + backward in write mode through the binding, then lr_densify_stats, view by view), and end to end through the
densify rule.

Tolerance of xyz_gradient_accum: the project's bar for the screen-space gradient (helpers.compare_grads: max|g - g_ref| <= 1e-4
max|g_ref|); a norm is 1-Lipschitz in its vector, so the bar of the vector carries over.  Rows of Gaussians that touch a pixel the
CPU oracle flags as threshold-fragile may be left out, within absgrad_cases.FRAGILE_ROW_CAP (tests/test_views_stats_cpu.py checks
the cap on the oracle alone).  denom and max_radii2D are exact everywhere."""
import ctypes

import numpy as np
import pytest
import torch

from luciddreamer_amd import _C, _lib, cameras, config, densify, parallel, synthetic
from tests import absgrad_cases as cases
from tests import absgrad_ref as ref
from tests import helpers as hp
from tests.test_views_stats_cpu import STAT_CASES, reference_stats

pytestmark = pytest.mark.gpu

EMPTY = torch.Tensor([])
MODES = ("grad", "absgrad")
ACC_SHAPES = lambda P, M: {"means3D": (P, 3), "means2D": (P, 3), "opacity": (P, 1), "sh": (P, M, 3), "scales": (P, 3),
                           "rotations": (P, 4)}


class _Switches:
    """The process-wide switches a case needs (the forward's anti-aliasing), restored on exit."""

    def __init__(self, case):
        self.case = case

    def __enter__(self):
        config.set_antialiasing(self.case["antialiasing"])

    def __exit__(self, *exc):
        config.set_antialiasing(False)
        return False


def _zero_stats(P, dev):
    return {"xyz_gradient_accum": torch.zeros(P, 1, device=dev), "denom": torch.zeros(P, 1, device=dev),
            "max_radii2D": torch.zeros(P, device=dev)}


def _run(batch, c, stats=None, acc=None):
    P, M = c["means3D"].shape[0], c["shs"].shape[1]
    acc = acc if acc is not None else {k: torch.zeros(s, device=c["means3D"].device) for k, s in ACC_SHAPES(P, M).items()}
    batch.run(c["means3D"], c["opacities"], c["scales"], c["rotations"], c["shs"], acc, stats=stats)
    return acc


def _forward(c, cam, bg, degree):
    """Exact-mode forward through the binding: (R, radii, geom, binning, img, depth, instances after exact tile culling)."""
    tfx, tfy = hp.tan_fov(cam)
    R, _, depth, radii, geom, binning, img = _C.rasterize_gaussians(
        bg, c["means3D"], EMPTY, c["opacities"], c["scales"], c["rotations"], 1.0, EMPTY, cam.world_view_transform,
        cam.full_proj_transform, tfx, tfy, cam.image_height, cam.image_width, c["shs"], degree, cam.camera_center, False, False)
    n_inst = int(geom[:32].cpu().numpy().view(np.uint32)[6])              # GeomHeader::num_instances
    return R, radii, geom, binning, img, depth, n_inst


def _per_view_route(c, cams, bg, degree, g_color, absgrad, stats):
    """The yardstick: per view, forward + backward in write mode (absgrad: with dL_dmean2D_abs), then lr_densify_stats, in order."""
    L = _lib.lib()
    P = c["means3D"].shape[0]
    dev = c["means3D"].device
    for cam in cams:
        tfx, tfy = hp.tan_fov(cam)
        R, radii, geom, binning, img, _, _ = _forward(c, cam, bg, degree)
        g = _C.rasterize_gaussians_backward(bg, c["means3D"], radii, EMPTY, c["scales"], c["rotations"], 1.0, EMPTY,
                                            cam.world_view_transform, cam.full_proj_transform, tfx, tfy, g_color, None, c["shs"],
                                            degree, cam.camera_center, geom, R, binning, img, False, absgrad=absgrad)
        G = g[8] if absgrad else dict(zip(_C.GRAD_ORDER, g[:8]))["means2D"]
        assert G.is_contiguous() and tuple(G.shape) == (P, 3)
        rc = L.lr_densify_stats(P, radii.data_ptr(), G.data_ptr(), stats["xyz_gradient_accum"].data_ptr(), stats["denom"].data_ptr(),
                                stats["max_radii2D"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    return stats


def _assert_norm_sum(got, want, what, rows=()):
    got = got.detach().double().cpu().numpy().reshape(-1).copy()
    want = np.asarray(want, dtype=np.float64).reshape(-1)
    got[list(rows)] = want[list(rows)]
    fig = hp.compare_grads({"accum": got}, {"accum": want}, names=["accum"])
    print(f"[views stats] {what}: max|a - a_ref| = {fig['accum'][0]:.3e}, max|a_ref| = {fig['accum'][1]:.3e}, rows left out {len(rows)}")


# ---- 1. against the float64 reference -----------------------------------------------------------------------------------------
def _case_on(case, dev):
    c = {k: v.to(dev) for k, v in case["cloud"].items()}
    t = lambda x, n: None if x is None else [x.to(dev)] * n
    return c, case["cam"].to(dev), case["bg"].to(dev), t


def _case_batch(case, dev, n_views, mode, n_streams=2):
    _, cam, bg, t = _case_on(case, dev)
    return parallel.ViewBatch([cam] * n_views, t(case["g_color"], n_views), cases.DEGREE, bg, binning_capacity=1 << 14,
                              n_streams=n_streams, grad_depths=t(case["g_depth"], n_views), grad_alphas=t(case["g_alpha"], n_views),
                              densify_stats=mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("name", STAT_CASES)
def test_against_the_float64_reference(hip_device, name, n_views, mode):
    case = cases.make(name)
    signed, absolute, vis = reference_stats(name)
    norm = absolute if mode == "absgrad" else signed
    rows, visible = ref.fragile_rows(name)
    assert len(rows) <= cases.FRAGILE_ROW_CAP * visible
    c, cam, bg, _ = _case_on(case, hip_device)
    P = vis.shape[0]
    # non-zero seeded contents: the step accumulates, and takes the max against what was there.  The norm sum starts within the
    # scale of what is added, so that the float32 rounding of the accumulation (2^-24 of the result) stays far below the bar
    gen = torch.Generator().manual_seed(17)
    a0 = (torch.rand(P, 1, generator=gen) * float(n_views * norm.max())).float()
    d0 = torch.randint(0, 5, (P, 1), generator=gen).float()
    m0 = torch.randint(0, 60, (P,), generator=gen).float()                # radii of these cases reach 19 .. 37: both sides of the max
    stats = {"xyz_gradient_accum": a0.to(hip_device), "denom": d0.to(hip_device), "max_radii2D": m0.to(hip_device)}
    with _Switches(case):
        radii = _forward(c, cam, bg, cases.DEGREE)[1].cpu().numpy()
        batch = _case_batch(case, hip_device, n_views, mode)
        _run(batch, c, stats)
        batch.check()
    assert np.array_equal(radii > 0, vis)
    added = stats["xyz_gradient_accum"].double().cpu() - a0.double()
    _assert_norm_sum(added, n_views * norm, f"{name} x{n_views} {mode}", rows)
    assert np.array_equal(stats["denom"].cpu().numpy()[:, 0], d0.numpy()[:, 0] + n_views * vis.astype(np.float32))
    assert np.array_equal(stats["max_radii2D"].cpu().numpy(), np.maximum(m0.numpy(), np.maximum(radii, 0).astype(np.float32)))
    assert P == 1 or ((m0.numpy() > radii).any() and (m0.numpy() < radii).any())


# ---- 2. / 4. against the per-view route on the same device --------------------------------------------------------------------
def _band_setup(dev, P, W, H, n_views, seed, path=None):
    """path: the rotate360 path's number of poses, of which the first n_views are taken (neighbouring poses of a 30-pose path
    share most of what they see; the default, n_views poses around the circle, share little)."""
    c = {k: v.to(dev) for k, v in synthetic.make_cloud(P, "band", seed).items()}
    cams = [cam.to(dev) for cam in cameras.rotate360_path(W, H, n_views=path or n_views)[:n_views]]
    return c, cams, synthetic.upstream_grad(H, W).to(dev), torch.tensor([0.1, 0.0, 0.2], device=dev)


def _step_stats(c, cams, g, bg, mode, n_streams, capacity):
    batch = parallel.ViewBatch(cams, [g] * len(cams), 3, bg, binning_capacity=capacity, n_streams=n_streams, densify_stats=mode)
    stats = _zero_stats(c["means3D"].shape[0], bg.device)
    acc = _run(batch, c, stats)
    batch.check()
    return stats, acc


def _assert_step_equals_per_view(step, per_view, what):
    assert torch.equal(step["denom"], per_view["denom"]), what
    assert torch.equal(step["max_radii2D"], per_view["max_radii2D"]), what
    assert float(per_view["denom"].sum()) > 0 and float(per_view["xyz_gradient_accum"].max()) > 0
    _assert_norm_sum(step["xyz_gradient_accum"], per_view["xyz_gradient_accum"].double().cpu().numpy(), what)


@pytest.mark.parametrize("mode", MODES)
def test_against_the_per_view_route_for_every_number_of_chains(hip_device, mode):
    P, W, H, cap = 3000, 72, 40, 200_000                                 # 72 x 40: partial tiles both ways
    c, cams, g, bg = _band_setup(hip_device, P, W, H, 5, seed=3)
    want = _per_view_route(c, cams, bg, 3, g, mode == "absgrad", _zero_stats(P, hip_device))
    plain = _run(parallel.ViewBatch(cams, [g] * 5, 3, bg, binning_capacity=cap, n_streams=2), c)
    stats, acc = _step_stats(c, cams, g, bg, mode, 2, cap)
    _assert_step_equals_per_view(stats, want, f"band 72x40 {mode}")
    assert float(plain["means2D"].abs().sum()) > 0
    if mode == "grad":
        for k in plain:                                                   # the step's gradients keep their bits
            assert torch.equal(acc[k], plain[k]), k
    # the same bits for every number of chains and every repeat -- with the blend shapes pinned, as in the step's other tests of
    # this property (tests/test_gpu_mask_views.py): left to itself the library picks a lone view's blend shape by the number of
    # views in flight, and another shape is another rounding of every gradient, signed sums included
    _lib.tune_set("blend_quad", 2)
    _lib.tune_set("fwd_pair", 2)
    try:
        first = None
        for n_streams in (1, 2, 3, 4):
            for rep in range(2):
                stats, _ = _step_stats(c, cams, g, bg, mode, n_streams, cap)
                first = first or stats
                for k in first:
                    assert torch.equal(stats[k], first[k]), (k, n_streams, rep)
        _assert_step_equals_per_view(first, want, f"band 72x40 {mode}, pinned shapes")
    finally:
        _lib.tune_set("blend_quad", -1)
        _lib.tune_set("fwd_pair", -1)


@pytest.mark.parametrize("mode", MODES)
def test_non_interleaved_accumulator_route(hip_device, mode):
    P, W, H, cap = 3000, 72, 40, 200_000
    c, cams, g, bg = _band_setup(hip_device, P, W, H, 5, seed=3)
    want = _per_view_route(c, cams, bg, 3, g, mode == "absgrad", _zero_stats(P, hip_device))
    inter, acc_i = _step_stats(c, cams, g, bg, mode, 2, cap)
    _lib.tune_set("gauss_bwd", 0)
    try:
        direct, acc_d = _step_stats(c, cams, g, bg, mode, 2, cap)
    finally:
        _lib.tune_set("gauss_bwd", -1)
    _assert_step_equals_per_view(direct, want, f"band 72x40 {mode}, rows accumulated in place")
    assert torch.equal(direct["denom"], inter["denom"]) and torch.equal(direct["max_radii2D"], inter["max_radii2D"])
    _assert_norm_sum(direct["xyz_gradient_accum"], inter["xyz_gradient_accum"].double().cpu().numpy(), f"{mode}: in place vs interleaved")
    for k in acc_i:
        hp.compare_grads({k: acc_d[k].double().cpu().numpy()}, {k: acc_i[k].double().cpu().numpy()}, names=[k])


# ---- 3. radii > 0 without a tile instance -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("offset", [0.8, 1.05])
def test_visible_gaussian_without_an_instance_counts(hip_device, mode, offset):
    case = cases.make("partial")
    cam = case["cam"]
    tfx, tfy = cases.tan_fov(cam)
    W, H = cam.image_width, cam.image_height
    r, z = 12.0, 3.0
    # 0.8: the 3 sigma square reaches tile (0, 0) and the 3 sigma disc misses the screen.  1.05: the same for the radius the
    # library itself gives this Gaussian (15: the 0.3 dilation and the clamped Jacobian off screen), should it keep the first one
    cx = cy = -offset * r
    assert np.hypot(cx, cy) > r + 1
    extra = dict(means3D=torch.tensor([[((2 * cx + 1) / W - 1) * tfx * z, ((2 * cy + 1) / H - 1) * tfy * z, z]]),
                 scales=torch.full((1, 3), (r / 3.0) * (2.0 * tfx / W) * z), rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]),
                 opacities=torch.tensor([[0.9]]), shs=torch.zeros(1, cases.SH_COEFFS, 3))
    base = {k: v.to(hip_device) for k, v in case["cloud"].items()}
    c = {k: torch.cat([v, extra[k].to(hip_device)]).contiguous() for k, v in base.items()}
    P, row = c["means3D"].shape[0], c["means3D"].shape[0] - 1
    camd, bg = cam.to(hip_device), case["bg"].to(hip_device)
    _, radii, _, _, _, _, n_with = _forward(c, camd, bg, cases.DEGREE)
    n_without = _forward(base, camd, bg, cases.DEGREE)[6]
    radii = radii.cpu().numpy()
    print(f"[views stats] extra Gaussian at {offset} r: radii {radii[row]}, owns {n_with - n_without} tile instance(s)")
    g = [case["g_color"].to(hip_device)] * 2
    batch = parallel.ViewBatch([camd] * 2, g, cases.DEGREE, bg, binning_capacity=1 << 14, n_streams=2, densify_stats=mode)
    stats = _zero_stats(P, hip_device)
    _run(batch, c, stats)
    batch.check()
    assert float(stats["denom"][row]) == (2.0 if radii[row] > 0 else 0.0)
    assert float(stats["max_radii2D"][row]) == float(max(radii[row], 0))
    if n_with == n_without:
        assert float(stats["xyz_gradient_accum"][row]) == 0.0
    assert np.array_equal(stats["denom"].cpu().numpy()[:, 0], 2.0 * (radii > 0))
    assert np.array_equal(stats["max_radii2D"].cpu().numpy(), np.maximum(radii, 0).astype(np.float32))
    assert not stats["xyz_gradient_accum"].cpu().numpy()[radii <= 0].any()


# ---- 5. the fused training step -----------------------------------------------------------------------------------------------
def test_fused_training_step_against_the_autograd_route(hip_device):
    from luciddreamer_amd.loss import alpha_hole, depth_l1, masked_l1_dssim
    from tests.test_gpu_mask_views import _depth_targets, _holey_targets, _render
    P, W, H, wa, wd = 2000, 64, 48, 0.6, 0.35
    c, cams, _, bg = _band_setup(hip_device, P, W, H, 4, seed=8, path=30)
    targets, masks = _holey_targets(hip_device, cams, W, H, 3)
    dts = _depth_targets(hip_device, cams, W, H, 70)
    leaf = {k: v.clone().requires_grad_(True) for k, v in c.items()}
    want_a, want_d, want_r = torch.zeros(P, device=hip_device), torch.zeros(P, device=hip_device), torch.zeros(P, device=hip_device)
    config.set_depth_gradient(True)
    try:
        for cam, tgt, m, dt in zip(cams, targets, masks, dts):
            m2d = torch.zeros(P, 3, device=hip_device, requires_grad=True)
            col, radii, dep, alp = _render(cam, W, H, bg, leaf, m2d)
            (masked_l1_dssim(col, tgt, m, 0.2) + wa * alpha_hole(alp, m) + wd * depth_l1(dep, dt)).backward()
            vis = radii > 0
            want_a += torch.where(vis, m2d.grad[:, :2].norm(dim=1), torch.zeros_like(want_a))
            want_d += vis.float()
            want_r = torch.maximum(want_r, radii.clamp(min=0).float())
    finally:
        config.set_depth_gradient(False)
    batch = parallel.ViewBatch(cams, None, 3, bg, binning_capacity=200_000, n_streams=2, targets=targets, lambda_dssim=0.2, masks=masks,
                               alpha_weight=wa, depth_targets=dts, depth_weight=wd, densify_stats="grad")
    stats = _zero_stats(P, hip_device)
    _run(batch, c, stats)
    batch.check()
    assert torch.equal(stats["denom"][:, 0], want_d) and torch.equal(stats["max_radii2D"], want_r)
    assert float(want_d.max()) > 1
    _assert_norm_sum(stats["xyz_gradient_accum"], want_a.double().cpu().numpy(), "fused training step")


# ---- 6. overflow ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_overflowed_view_contributes_nothing(hip_device, mode):
    P, W, H = 3000, 72, 40
    c, cams, g, bg = _band_setup(hip_device, P, W, H, 3, seed=3, path=30)
    counts = [_forward(c, cam, bg, 3)[6] for cam in cams]
    order = np.argsort(counts)
    lost, second = int(order[-1]), counts[order[-2]]
    assert second < counts[lost], counts
    cap = (second + counts[lost]) // 2                   # second <= cap < the largest: exactly one view overflows
    print(f"[views stats] instances per view {counts}, capacity {cap}: view {lost} overflows")
    batch = parallel.ViewBatch(cams, [g] * 3, 3, bg, binning_capacity=cap, n_streams=2, densify_stats=mode)
    stats = _zero_stats(P, hip_device)
    _run(batch, c, stats)
    with pytest.raises(RuntimeError, match="capacity"):
        batch.check()
    kept = [cam for i, cam in enumerate(cams) if i != lost]
    want, _ = _step_stats(c, kept, g, bg, mode, 2, 200_000)
    assert torch.equal(stats["denom"], want["denom"]) and torch.equal(stats["max_radii2D"], want["max_radii2D"])
    assert float(want["denom"].max()) == 2.0
    _assert_norm_sum(stats["xyz_gradient_accum"], want["xyz_gradient_accum"].double().cpu().numpy(), f"overflow {mode}")


# ---- 7. the densify rule, end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_densify_rule_on_the_cancellation_case_in_a_step(hip_device, mode):
    """The multi-view twin of tests/test_gpu_absgrad.py::test_densify_rule_on_the_cancellation_case: two views of the broad
    Gaussian whose per-pixel pulls cancel; at the reference's threshold "absgrad" selects it and "grad" does not."""
    from tests.test_gpu_absgrad import _model
    case = cases.make("cancel")
    m = _model(case, hip_device)
    c = {k: v.to(hip_device) for k, v in case["cloud"].items()}
    stats = densify.view_batch_stats(m)
    assert stats["xyz_gradient_accum"] is m.xyz_gradient_accum and stats["max_radii2D"] is m.max_radii2D
    batch = _case_batch(case, hip_device, 2, mode)
    _run(batch, c, stats)
    batch.check()
    assert float(m.denom[0]) == 2.0
    print(f"[views stats] cancel, {mode}: mean statistic {float(m.xyz_gradient_accum[0] / m.denom[0]):.3e}")
    densify.densify_and_prune(m, 0.0002, 0.005, 10.0, None)
    assert m._xyz.shape[0] == (2 if mode == "absgrad" else 1)


# ---- 8. one mid-size step: several chains, several workgroups -----------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_mid_size_step_against_the_per_view_route(hip_device, mode):
    P, W, H = 200_000, 512, 512
    c, cams, g, bg = _band_setup(hip_device, P, W, H, 6, seed=1)
    counts = [_forward(c, cam, bg, 3)[6] for cam in cams]
    want = _per_view_route(c, cams, bg, 3, g, mode == "absgrad", _zero_stats(P, hip_device))
    stats, _ = _step_stats(c, cams, g, bg, mode, 3, int(1.25 * max(counts)) + 4096)
    _assert_step_equals_per_view(stats, want, f"200 k, 512^2, 6 views, {mode}")


# ---- 9. the example loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("absgrad", [False, True], ids=MODES)
def test_example_loop_densifies_on_the_step_statistics(hip_device, absgrad):
    """examples/train_loop.py --multi-view 3: one ViewBatch step with targets per iteration, Adam, densify_and_prune on the
    statistics the step itself accumulated: the loss falls and the number of Gaussians changes."""
    import importlib.util
    import math
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "train_loop.py")
    spec = importlib.util.spec_from_file_location("train_loop_example_mv", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.default_args(gaussians=6000, iters=40, resolution="128x96", views=6, log=10, densify_from=20, densify_every=20,
                            multi_view=3, absgrad=absgrad, densify_grad_threshold=0.0008 if absgrad else 0.0002)
    losses, _ = mod.train(args, log=lambda s: None)
    assert all(math.isfinite(l) for _, l, _ in losses)
    assert losses[-1][1] < losses[0][1], losses
    assert len({p for _, _, p in losses}) > 1, "densify_and_prune never changed the number of Gaussians"
