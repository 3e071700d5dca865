"""Normals from depth and the normal losses on the GPU (luciddreamer_amd.normals -> lr_depth_normals*, lr_normal_loss_*).

The kernels against the float64 lifted-point reference of tests/normal_ref.py (its own properties: tests/test_normals_cpu.py), with
the float32 restatement of the header's closed form as the calibrator of every bar:

    normals   max|n - n64| <= max(4 e32, 16 * 2^-24)        e32: the restatement's own distance from float64 on that case,
                                                            4 = rowbar.E32_MARGIN, 16 roundings between a depth and a component
    value     |loss - loss64| <= 1e-6                       the sister kernels' bar; the count is exact
    gradient  max|g - g64| <= max(4 e32_grad, 1e-6 max|g64|), zero where the reference is zero, and rowbar.judge with pixels as
              rows, no fragile rows and two float32 calibrators (the header's gather order and its reverse) reports no failure

then bit-repeatability, the [1,H,W] / [H,W] forms, the upstream scalar, scale invariance, a tilted plane, the consistency term of
a depth with itself, and both terms through the rasterizer's depth and median-depth gradients.  Every test fails without the
feature: luciddreamer_amd.normals does not exist there."""
import functools

import numpy as np
import pytest
import torch

from luciddreamer_amd import config
from tests import helpers as hp, normal_ref as nr, rowbar

pytestmark = pytest.mark.gpu

TX, TY = nr.TAN
CAM = nr.TAN
WEIGHT = 0.7
FLOOR = 16 * 2.0 ** -24
# (3,3) one interior pixel; (5,7); (16,16) one ragged workgroup; (67,131) ragged, several workgroups in both directions;
# (257,511); (600,900): 2 110 workgroup partials, more than the final workgroup has threads
SHAPES = [(3, 3), (5, 7), (16, 16), (67, 131), (257, 511), (600, 900)]
DEGENERATE = [(2, 9), (9, 2)]
MODES = [("smooth", "target"), ("rand", "target"), ("smooth", "consistency")]


def _seed(H, W):
    return 1000 * H + W


@functools.lru_cache(maxsize=None)
def _case(H, W, kind):
    return nr.make_case(H, W, _seed(H, W), kind)


def _target(case, mode):
    return dict(target_depth=case["depth_b"]) if mode == "consistency" else dict(target_normals=case["target_normals"])


@functools.lru_cache(maxsize=None)
def _refs(H, W, kind, mode, with_weight, upstream=1.0):
    """(float64 reference, float32 calibrator in the header's order, ... in the reverse order), computed once per case."""
    case = _case(H, W, kind)
    r = nr.reference(case, TX, TY, mode, with_weight, WEIGHT)
    kw = dict(pixel_weight=case["pixel_weight"] if with_weight else None, weight=WEIGHT, upstream=upstream, **_target(case, mode))
    a = nr.closed_form(case["depth"], TX, TY, np.float32, order="WENS", **kw)
    b = nr.closed_form(case["depth"], TX, TY, np.float32, order="SNEW", **kw)
    return r, a, b


def _device_loss(case, dev, mode, with_weight, upstream=1.0, lead=False, grad_b=True):
    """(loss, count, grad, grad of depth_b or None) of the device kernels through the Python module."""
    from luciddreamer_amd import normals
    up = lambda t: torch.from_numpy(t[None] if lead else t).to(dev)
    d = up(case["depth"]).requires_grad_(True)
    pw = up(case["pixel_weight"]) if with_weight else None
    if mode == "consistency":
        t = up(case["depth_b"]).requires_grad_(grad_b)
        loss = normals.normal_consistency(d, t, CAM, pw, WEIGHT)
    else:
        t = torch.from_numpy(case["target_normals"]).to(dev)
        loss = normals.normal_loss(d, t, CAM, pw, WEIGHT)
    count = normals.normal_count(d, t, CAM, pw)
    (loss * upstream if upstream != 1.0 else loss).backward()
    return loss.detach(), count, d.grad, (t.grad if mode == "consistency" else None)


def _gradient_bar(got, r64, a32, b32, what):
    """The issue's gradient bar of one [H,W] gradient; prints the figures first."""
    got = got.astype(np.float64)
    gmax = np.abs(r64).max()
    e32 = max(np.abs(a32 - r64).max(), np.abs(b32 - r64).max())
    err = np.abs(got - r64).max()
    bits = bool(np.array_equal(got.astype(np.float32).view(np.uint32), a32.view(np.uint32)))
    print(f"[normals] {what}: gradient max|g - g64| {err:.3e} = {err / gmax if gmax else 0:.2e} of max|g64| {gmax:.3e}; "
          f"float32 restatements within {e32:.3e} = {e32 / gmax if gmax else 0:.2e}; bit-equal to the header-order restatement: {bits}")
    assert np.isfinite(got).all()
    assert err <= max(rowbar.E32_MARGIN * e32, 1e-6 * gmax), (what, err, e32, gmax)
    assert not got[r64 == 0].any(), what                                   # corners, pixels without a counted neighbour
    col = lambda g: np.asarray(g).reshape(-1, 1)
    rep = rowbar.judge(col(got), col(r64), [col(a32), col(b32)])
    assert not rep["failed"], (what, len(rep["failed"]), rep["failed"][:3])
    return err, e32


# ---- 1. the kernels against the references --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind", ["smooth", "rand"])
def test_normals_match_the_float64_reference(hip_device, H, W, kind):
    from luciddreamer_amd import normals
    case = _case(H, W, kind)
    n64, valid = nr.torch_normals(torch.from_numpy(case["depth"].astype(np.float64)), TX, TY)
    n64, valid = n64.numpy(), valid.numpy()
    n32, v32 = nr.closed_normals(case["depth"], TX, TY, np.float32)
    assert valid.any() and np.array_equal(valid, v32)
    e32 = np.abs(n32 - n64).max()
    d = torch.from_numpy(case["depth"]).to(hip_device)
    got_t = normals.depth_normals(d, CAM)
    got = got_t.cpu().numpy()
    err = np.abs(got - n64).max()
    print(f"[normals] {H}x{W} {kind}: max|n - n64| {err:.3e}, float32 restatement within {e32:.3e}, "
          f"bit-equal to it: {bool(np.array_equal(got.view(np.uint32), n32.view(np.uint32)))}")
    assert tuple(got.shape) == (3, H, W) and np.isfinite(got).all()
    assert err <= max(rowbar.E32_MARGIN * e32, FLOOR)
    assert not got[:, ~valid].any()                                        # invalid pixels are exactly (0,0,0) ...
    assert np.array_equal((got != 0).any(axis=0), valid)                   # ... and the validity pattern is the reference's
    # a [1,H,W] depth gives the same bits; so does 2 * depth (exact by construction)
    assert torch.equal(normals.depth_normals(d[None], CAM), got_t)
    assert torch.equal(normals.depth_normals(d * 2.0, CAM), got_t)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("with_weight", [True, False], ids=["weights", "no_weights"])
@pytest.mark.parametrize("kind,mode", MODES)
def test_loss_and_gradient_match_the_float64_reference(hip_device, H, W, kind, mode, with_weight):
    case = _case(H, W, kind)
    r, a, b = _refs(H, W, kind, mode, with_weight)
    # the condition, on the reference, before the device is asked
    assert nr.counted_fraction(r, H, W) >= nr.MIN_COUNTED and a["count"] == r["count"]
    loss, count, g, gt = _device_loss(case, hip_device, mode, with_weight)
    what = f"{H}x{W} {kind} {mode} {'weights' if with_weight else 'no weights'}"
    print(f"[normals] {what}: loss {float(loss):.8f} want {r['value']:.8f} |diff| {abs(float(loss) - r['value']):.2e} "
          f"(float32 restatement {abs(a['value'] - r['value']):.2e}); counted {int(count)} of {H * W}")
    assert abs(float(loss) - r["value"]) <= 1e-6
    assert float(count) == r["count"]
    assert tuple(g.shape) == (H, W)
    _gradient_bar(g.cpu().numpy(), r["grad"], a["grad"], b["grad"], what)
    if mode == "consistency":
        _gradient_bar(gt.cpu().numpy(), r["grad_target"], a["grad_target"], b["grad_target"], what + " (second depth)")


@pytest.mark.parametrize("H,W", SHAPES)
def test_vjp_of_the_normals_matches_the_float64_reference(hip_device, H, W):
    from luciddreamer_amd import normals
    case = _case(H, W, "smooth")
    Gn = np.random.default_rng(7).standard_normal((3, H, W)).astype(np.float32)
    r = nr.reference_vjp(case["depth"], Gn, TX, TY)
    a = nr.closed_form_vjp(case["depth"], Gn, TX, TY, np.float32, "WENS")
    b = nr.closed_form_vjp(case["depth"], Gn, TX, TY, np.float32, "SNEW")
    d = torch.from_numpy(case["depth"]).to(hip_device).requires_grad_(True)
    (normals.depth_normals(d, CAM) * torch.from_numpy(Gn).to(hip_device)).sum().backward()
    _gradient_bar(d.grad.cpu().numpy(), r, a, b, f"{H}x{W} depth_normals backward")


@pytest.mark.parametrize("H,W", DEGENERATE)
def test_an_image_without_an_interior_gives_exact_zeros(hip_device, H, W):
    from luciddreamer_amd import normals
    case = _case(H, W, "smooth")
    assert not normals.depth_normals(torch.from_numpy(case["depth"]).to(hip_device), CAM).any()
    for mode in ("target", "consistency"):
        for with_weight in (True, False):
            loss, count, g, gt = _device_loss(case, hip_device, mode, with_weight, upstream=1.3)
            assert float(loss) == 0.0 and float(count) == 0.0 and not g.any() and (gt is None or not gt.any())


# ---- 2. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(67, 131), (600, 900)])
@pytest.mark.parametrize("mode", ["target", "consistency"])
def test_repeated_calls_forms_and_upstream(hip_device, H, W, mode):
    case = _case(H, W, "smooth")
    first = _device_loss(case, hip_device, mode, True, upstream=1.3)
    for _ in range(4):                                                    # five calls: equal bits, value and gradient
        again = _device_loss(case, hip_device, mode, True, upstream=1.3)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]) and torch.equal(again[2], first[2])
        assert mode == "target" or torch.equal(again[3], first[3])
    lead = _device_loss(case, hip_device, mode, True, upstream=1.3, lead=True)           # [1,H,W] inputs
    assert tuple(lead[2].shape) == (1, H, W)
    assert torch.equal(lead[0], first[0]) and torch.equal(lead[2][0], first[2])
    assert mode == "target" or torch.equal(lead[3][0], first[3])
    # the upstream scalars are honoured: 1.3 and -2.0 against the reference scaled by them
    for up, got in ((1.3, first), (-2.0, _device_loss(case, hip_device, mode, True, upstream=-2.0))):
        r, a, b = _refs(H, W, "smooth", mode, True, up)
        _gradient_bar(got[2].cpu().numpy(), up * r["grad"], a["grad"], b["grad"], f"{H}x{W} {mode} upstream {up}")
    if mode == "consistency":
        # a depth passed detached gets no gradient, and the other one's does not change
        alone = _device_loss(case, hip_device, mode, True, upstream=1.3, grad_b=False)
        assert alone[3] is None and torch.equal(alone[2], first[2])


# ---- 3. analytic cases -------------------------------------------------------------------------------------------------------------
def test_a_tilted_plane_has_its_own_normal_everywhere(hip_device):
    """d = -k / (n0 . (u, v, 1)) is the plane n0 . X = -k seen from the origin: every interior normal is n0.  The bar: the
    forward bar plus the float64 reference's own distance from n0 on the float32-rounded depths (input rounding alone)."""
    from luciddreamer_amd import normals
    H, W = 33, 47
    n0 = np.array([0.35, -0.25, -1.0])
    n0 /= np.linalg.norm(n0)
    u = (np.arange(W) + 0.5) * (2 * TX / W) - TX
    v = (np.arange(H) + 0.5) * (2 * TY / H) - TY
    den = n0[0] * u[None, :] + n0[1] * v[:, None] + n0[2]
    assert (den < 0).all()
    depth = (-3.0 / den).astype(np.float32)
    n64, valid = nr.torch_normals(torch.from_numpy(depth.astype(np.float64)), TX, TY)
    n64, valid = n64.numpy(), valid.numpy()
    assert valid[1:-1, 1:-1].all() and valid.sum() == (H - 2) * (W - 2)
    own = np.abs(n64[:, 1:-1, 1:-1] - n0[:, None, None]).max()
    e32 = np.abs(nr.closed_normals(depth, TX, TY, np.float32)[0] - n64).max()
    got = normals.depth_normals(torch.from_numpy(depth).to(hip_device), CAM).cpu().numpy()
    err = np.abs(got[:, 1:-1, 1:-1] - n0[:, None, None]).max()
    print(f"[normals] tilted plane {H}x{W}: max|n - n0| {err:.3e}; float64 reference from n0 {own:.3e}; float32 restatement {e32:.3e}")
    assert err <= max(rowbar.E32_MARGIN * e32, FLOOR) + own


@pytest.mark.parametrize("H,W", [(67, 131), (257, 511)])
def test_a_depth_is_consistent_with_itself(hip_device, H, W):
    from luciddreamer_amd import normals
    case = _case(H, W, "smooth")
    same = dict(case, depth_b=case["depth"])
    r = nr.reference(same, TX, TY, "consistency", False, WEIGHT)
    a = nr.closed_form(case["depth"], TX, TY, np.float32, target_depth=case["depth"], weight=WEIGHT)
    assert r["count"] > 0 and np.abs(r["grad"]).max() <= 1e-15
    bar = max(rowbar.E32_MARGIN * np.abs(a["grad"] - r["grad"]).max(), 1e-6 * np.abs(r["grad"]).max())
    d = torch.from_numpy(case["depth"]).to(hip_device).requires_grad_(True)
    loss = normals.normal_consistency(d, d.detach().clone().requires_grad_(True), CAM, None, WEIGHT)
    loss.backward()
    g = np.abs(d.grad.cpu().numpy()).max()
    print(f"[normals] {H}x{W} consistency of a depth with itself: value {float(loss.detach()):.3e}, max|gradient| {g:.3e}, bar {bar:.3e}")
    assert abs(float(loss.detach())) <= 4 * 2.0 ** -24 * WEIGHT
    assert float(normals.normal_count(d, d.detach(), CAM)) == r["count"]
    assert g <= bar


# ---- 4. through the rasterizer ---------------------------------------------------------------------------------------------------
NAMES = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
RW, RH, RP = 64, 64, 400


@pytest.fixture
def depth_on():
    config.set_depth_gradient(True)
    yield
    config.set_depth_gradient(False)


@pytest.fixture
def exact_mode():
    """Bit comparisons between calls: every forward in exact mode (async mode's binning bound can pick another shape)."""
    config.set_async(False)
    yield
    config.set_async(True)
    config.reset()


def _render(cloud, cam, dev, median=False):
    """(leaves, outputs) of GaussianRasterizer on fresh leaves."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    tfx, tfy = hp.tan_fov(cam)
    c = cam.to(dev)
    rs = GaussianRasterizationSettings(cam.image_height, cam.image_width, tfx, tfy, torch.zeros(3, device=dev), 1.0,
                                       c.world_view_transform, c.full_proj_transform, 1, c.camera_center, False, False)
    leaves = {k: cloud[k].detach().to(dev).requires_grad_(True) for k in NAMES if k != "means2D"}
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
    out = GaussianRasterizer(rs)(**leaves, **(dict(return_median=True) if median else {}))
    return leaves, out


def _grads(leaves):
    return {k: (torch.zeros_like(t) if t.grad is None else t.grad.clone()) for k, t in leaves.items()}


def test_normal_loss_through_the_rasterizer_is_the_depth_gradient_of_the_reference(hip_device, depth_on):
    """normal_loss(depth, t).backward() against depth.backward(g), g the float64 reference's gradient on the rendered depth cast to
    float32: both sides run the same rasterizer backward.  The bar of tests/test_gpu_depth_views.py: 2e-5 of each tensor's maximum."""
    from luciddreamer_amd import normals
    cam, cloud = hp.box_setup(RP, RW, RH, scale_mult=2.0)
    t_np = _case(RH, RW, "smooth")["target_normals"]
    t = torch.from_numpy(t_np).to(hip_device)
    leaves, out = _render(cloud, cam, hip_device)
    depth = out[2]
    assert tuple(depth.shape) == (1, RH, RW) and depth.requires_grad
    d_np = depth.detach().cpu().numpy()[0]
    r = nr.reference(dict(depth=d_np, target_normals=t_np), *hp.tan_fov(cam), "target", False, WEIGHT)
    print(f"[normals] rasterizer {RH}x{RW}, {RP} Gaussians: {r['count']} pixels counted, loss {r['value']:.6f}")
    assert r["count"] >= 0.25 * RH * RW and np.abs(r["grad"]).max() > 0
    loss = normals.normal_loss(depth, t, cam, None, WEIGHT)
    assert abs(float(loss.detach()) - r["value"]) <= 1e-6
    loss.backward()
    got = _grads(leaves)
    leaves2, out2 = _render(cloud, cam, hip_device)
    out2[2].backward(torch.from_numpy(r["grad"].astype(np.float32))[None].to(hip_device))
    want = _grads(leaves2)
    for k in NAMES:
        a, b = got[k].cpu().numpy(), want[k].cpu().numpy()
        scale = np.abs(b).max()
        err = np.abs(a - b).max()
        print(f"[normals] rasterizer {k}: max|g - g_ref| {err:.3e} of max {scale:.3e}")
        if k == "shs":                                                    # the depth does not depend on the colours
            assert not a.any() and not b.any()
            continue
        assert np.isfinite(a).all() and scale > 0 and err <= 2e-5 * scale, (k, err, scale)


def test_consistency_of_depth_and_median_depth_through_the_rasterizer(hip_device, depth_on, exact_mode):
    """normal_consistency(depth, median_depth): the median's gradient reaches the means alone, so opacity, scale and rotation get
    the expected depth's side only -- the bits of the same call with the median passed detached."""
    from luciddreamer_amd import normals
    cam, cloud = hp.box_setup(RP, RW, RH, scale_mult=2.0)

    def once(detach):
        leaves, out = _render(cloud, cam, hip_device, median=True)
        depth, median = out[2], out[-2]
        assert tuple(median.shape) == (1, RH, RW)
        loss = normals.normal_consistency(depth, median.detach() if detach else median, cam, None, WEIGHT)
        count = float(normals.normal_count(depth, median, cam))
        loss.backward()
        return float(loss), count, _grads(leaves)

    loss, count, both = once(False)
    loss_d, _, alone = once(True)
    print(f"[normals] rasterizer consistency: loss {loss:.6f}, {int(count)} pixels counted, "
          f"max|dL/dmeans3D| {float(both['means3D'].abs().max()):.3e} (median detached: {float(alone['means3D'].abs().max()):.3e})")
    assert loss == loss_d and loss > 0 and count >= 0.1 * RH * RW
    assert bool(torch.isfinite(both["means3D"]).all()) and float(both["means3D"].abs().max()) > 0
    assert not torch.equal(both["means3D"], alone["means3D"])             # the median's side is there ...
    for k in ("opacities", "scales", "rotations"):                        # ... and reaches nothing else
        assert float(alone[k].abs().max()) > 0 and torch.equal(both[k], alone[k]), k


# ---- 5. the example loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [dict(normal_weight=0.05), dict(normal_consistency=0.05),
                                   dict(normal_weight=0.05, normal_consistency=0.05)], ids=["normal", "consistency", "both"])
def test_example_loop_with_the_normal_terms(hip_device, flags):
    import importlib.util
    import math
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_loop_example_normals_gpu", os.path.join(root, "examples", "train_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    plain, _ = mod.train(mod.default_args(gaussians=2000, iters=20, resolution="64x64", log=1), log=lambda s: None)
    losses, _ = mod.train(mod.default_args(gaussians=2000, iters=20, resolution="64x64", log=1, **flags), log=lambda s: None)
    assert len(losses) == 20 and all(math.isfinite(l) for _, l, _ in losses)
    assert losses[0][1] > plain[0][1]                   # the term is in the loss from the first iteration on
    assert not config.depth_gradient()                  # the loop leaves the switch as it found it
