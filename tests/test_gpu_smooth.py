"""Edge-aware smoothness of a rendered map on the GPU (luciddreamer_amd.smooth -> lr_smooth_forward / lr_smooth_backward).

The kernels against the float64 reference of tests/smooth_ref.py (its own properties: tests/test_smooth_cpu.py), with the float32
restatements of the header's operations -- the gather in the header's order and in its reverse -- as the calibrators of every bar:

    value     |loss - loss64| <= max(4 e32_loss, 1e-6)      e32_loss: the restatement's own distance from float64 on that case,
                                                            4 = rowbar.E32_MARGIN; the count is exact
    gradient  max|g - g64| <= max(4 e32, 1e-6 max|g64|)     the 1e-6 floor is the sister kernels' and covers the device's expf
                                                            against numpy's; exact zeros wherever the reference is zero; and
              rowbar.judge with pixels as rows, no fragile rows and both restatements as calibrators reports no failure

on the piecewise-constant guide of smooth_ref.make_case; under its textured guide the gradient is held to the first of the two
gradient bars alone (neighbouring float32 weights cancel there: smooth_ref.make_case says why).  Then bit-repeatability, the
[1,H,W] / [H,W] forms, the upstream scalar, gamma = 0 against no guide, and the term on the
rasterizer's depth output.  Every test fails without the feature: luciddreamer_amd.smooth does not exist there."""
import functools

import numpy as np
import pytest
import torch

from luciddreamer_amd import config
from tests import helpers as hp, rowbar, smooth_ref as sr

pytestmark = pytest.mark.gpu

# (1,1) no term; (1,2), (2,1) a single pair; (2,9), (9,2) order 2 has terms in one direction only; (3,3); (5,7); (16,16) one
# ragged workgroup; (67,131) ragged, several workgroups both ways; (257,511); (600,900): 570 workgroup partials, more than the
# final workgroup has threads
SHAPES = [(1, 1), (1, 2), (2, 1), (2, 9), (9, 2), (3, 3), (5, 7), (16, 16), (67, 131), (257, 511), (600, 900)]
MIDDLE = [(3, 3), (5, 7), (16, 16)]


def _seed(H, W):
    return 1000 * H + W


@functools.lru_cache(maxsize=None)
def _case(H, W, kind):
    return sr.make_case(H, W, _seed(H, W), kind)


def _kw(case, what, order, space, guided, gamma=sr.GAMMA, guide="guide"):
    """(the map [C,H,W], the keyword arguments of the references)."""
    x = case["vectors"] if what == "vectors" else case["depth"][None]
    return x, dict(guide=case[guide] if guided else None, mask=case["mask"] if guided else None, order=order, space=space,
                   positive_only=what != "vectors", gamma=gamma, weight=sr.WEIGHT)


@functools.lru_cache(maxsize=None)
def _refs(H, W, kind, what, order, space, guided, upstream=1.0, guide="guide"):
    """(float64 reference, float32 restatement in the header's gather order, ... in the reverse order), once per case."""
    x, kw = _kw(_case(H, W, kind), what, order, space, guided, guide=guide)
    return (sr.reference(x, upstream=upstream, **kw), sr.restate32(x, upstream=upstream, **kw),
            sr.restate32(x, upstream=upstream, gather="reverse", **kw))


def _device(case, dev, what, order, space, guided, upstream=1.0, flat=False, gamma=sr.GAMMA, guide="guide"):
    """(loss, count, gradient) of the device kernels through the Python module; flat: the depth as [H,W]; guide: the case's
    image to guide by, None for the mask alone."""
    from luciddreamer_amd import smooth
    up = lambda t: torch.from_numpy(t).to(dev)
    image = up(case[guide]) if guided and guide else None
    mask = up(case["mask"]) if guided else None
    if what == "vectors":
        x = up(case["vectors"]).requires_grad_(True)
        loss = smooth.map_smoothness(x, image, order=order, gamma=gamma, weight=sr.WEIGHT, mask=mask)
        count = smooth.smoothness_count(x, image, order=order, mask=mask)
    else:
        x = up(case["depth"] if flat else case["depth"][None]).requires_grad_(True)
        loss = smooth.depth_smoothness(x, image, order=order, space=space, gamma=gamma, weight=sr.WEIGHT, mask=mask)
        count = smooth.smoothness_count(x, image, order=order, space=space, mask=mask, depth=True)
    assert loss.dim() == 0 and count.dim() == 0 and not count.requires_grad
    (loss * upstream if upstream != 1.0 else loss).backward()
    return loss.detach(), count, x.grad


def _gradient_bar(got, r64, a32, b32, what, per_pixel=True):
    """The gradient bars of one [C,H,W] gradient; prints the figures first."""
    got = got.astype(np.float64)
    gmax = np.abs(r64).max()
    e32 = max(np.abs(a32 - r64).max(), np.abs(b32 - r64).max())
    err = np.abs(got - r64).max()
    bits = bool(np.array_equal(got.astype(np.float32), a32))
    print(f"[smooth] {what}: gradient max|g - g64| {err:.3e} = {err / gmax if gmax else 0:.2e} of max|g64| {gmax:.3e}; "
          f"float32 restatements within {e32:.3e} = {e32 / gmax if gmax else 0:.2e}; equal to the header-order restatement: {bits}")
    assert np.isfinite(got).all()
    assert err <= max(rowbar.E32_MARGIN * e32, 1e-6 * gmax), (what, err, e32, gmax)
    assert not got[r64 == 0].any(), what                                   # invalid pixels, pixels without a counted term
    if not per_pixel:
        return
    rows = lambda g: np.asarray(g).reshape(g.shape[0], -1).T               # pixels as rows, channels as columns
    rep = rowbar.judge(rows(got), rows(r64), [rows(a32), rows(b32)])
    print(f"[smooth] {what}: per-pixel judge: worst err / pixel max {rep['worst']:.2e}, {rep['above_floor']} of {rep['rows']} pixels "
          f"above the {hp.GRAD_RTOL:g} floor, {len(rep['failed'])} failed")
    assert not rep["failed"] and not rep["excused"], (what, len(rep["failed"]), rep["failed"][:3])


def _check(dev, H, W, kind, what, order, space, guided):
    case = _case(H, W, kind)
    r, a, b = _refs(H, W, kind, what, order, space, guided)
    loss, count, g = _device(case, dev, what, order, space, guided)
    tag = f"{H}x{W} {kind} {what} order {order} {space} {'guide+mask' if guided else 'plain'}"
    e32_loss = abs(a["value"] - r["value"])
    print(f"[smooth] {tag}: loss {float(loss):.8f} want {r['value']:.8f} |diff| {abs(float(loss) - r['value']):.2e} "
          f"(float32 restatement {e32_loss:.2e}); counted {int(count)} terms, reference {r['count']}")
    assert abs(float(loss) - r["value"]) <= max(rowbar.E32_MARGIN * e32_loss, 1e-6)
    assert float(count) == r["count"] == a["count"]
    assert tuple(g.shape) == r["grad"].shape
    if r["count"] == 0:
        assert float(loss) == 0.0 and not g.any()
        return
    _gradient_bar(g.cpu().numpy(), r["grad"], a["grad"], b["grad"], tag)


# ---- 1. the kernels against the references --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("guided", [True, False], ids=["guide_mask", "plain"])
@pytest.mark.parametrize("space", ["depth", "inverse"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("kind", ["smooth", "rand"])
def test_depth_smoothness_matches_the_float64_reference(hip_device, H, W, kind, order, space, guided):
    r = _refs(H, W, kind, "depth", order, space, guided)[0]
    # the condition, on the reference, before the device is asked
    if (H, W) == (1, 1) or (order == 2 and max(H, W) < 3):
        assert r["count"] == 0
    elif (H, W) in ((1, 2), (2, 1)) and order == 1:
        assert r["count"] == 1
    elif (H, W) in ((2, 9), (9, 2)) and order == 2:
        assert r["count"] == 2 * 7 and (r["counted_x"].size == 0 or r["counted_y"].size == 0)
    else:
        assert r["count"] >= (0.5 if H * W >= 64 else 1.0) * ((H - order) * W + H * (W - order))
    _check(hip_device, H, W, kind, "depth", order, space, guided)


@pytest.mark.parametrize("H,W", MIDDLE)
@pytest.mark.parametrize("guided", [True, False], ids=["guide_mask", "plain"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("kind", ["smooth", "rand"])
def test_map_smoothness_of_three_channels_matches_the_float64_reference(hip_device, H, W, kind, order, guided):
    assert _refs(H, W, kind, "vectors", order, "depth", guided)[0]["count"] > 0
    _check(hip_device, H, W, kind, "vectors", order, "depth", guided)


@pytest.mark.parametrize("H,W", [(67, 131), (257, 511)])
@pytest.mark.parametrize("order,space", [(1, "depth"), (2, "depth"), (2, "inverse")])
def test_a_textured_guide_is_held_to_the_scale_of_the_gradient(hip_device, H, W, order, space):
    """Every term has a weight of its own here (expf at as many arguments as there are terms).  Value, count, zeros and the
    tensor-scale gradient bar; not the per-pixel judge: where a pixel's float32 weights cancel, its digits are the expf's."""
    case = _case(H, W, "smooth")
    r, a, b = _refs(H, W, "smooth", "depth", order, space, True, guide="texture")
    loss, count, g = _device(case, hip_device, "depth", order, space, True, guide="texture")
    e32_loss = abs(a["value"] - r["value"])
    print(f"[smooth] {H}x{W} textured guide order {order} {space}: loss {float(loss):.8f} want {r['value']:.8f} "
          f"(float32 restatement {e32_loss:.2e}); counted {int(count)}")
    assert abs(float(loss) - r["value"]) <= max(rowbar.E32_MARGIN * e32_loss, 1e-6) and float(count) == r["count"]
    _gradient_bar(g.cpu().numpy(), r["grad"], a["grad"], b["grad"], f"{H}x{W} textured guide order {order} {space}", per_pixel=False)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("gamma", [0.0, sr.GAMMA])
def test_a_subnormal_depth_and_an_infinite_guide_value_exclude_their_terms(hip_device, order, gamma):
    """INVERSE space: a depth of 1e-40 is > 0 and finite, its float32 reciprocal is not, so the pixel is invalid.  A guide value
    of +inf makes the guide difference of its terms infinite: they do not count, at gamma = 0 (where the weight would be
    expf(-(0 inf)) = NaN) as at any other.  Value, count and every gradient stay finite and meet the bars."""
    from luciddreamer_amd import smooth
    H, W = 9, 11
    base = _case(H, W, "rand")
    depth, guide = base["depth"].copy(), base["guide"].copy()
    depth[4, 5] = np.float32(1e-40)
    guide[:, 2, 3] = np.inf
    kw = dict(guide=guide, order=order, space="inverse", positive_only=True, gamma=gamma, weight=sr.WEIGHT)
    r, a, b = sr.reference(depth[None], **kw), sr.restate32(depth[None], **kw), sr.restate32(depth[None], gather="reverse", **kw)
    plain = sr.reference(base["depth"][None], **dict(kw, guide=base["guide"]))
    assert not r["valid"][4, 5] and 0 < r["count"] < plain["count"] and np.isfinite(r["value"])
    d = torch.from_numpy(depth).to(hip_device).requires_grad_(True)
    image = torch.from_numpy(guide).to(hip_device)
    loss = smooth.depth_smoothness(d, image, order=order, space="inverse", gamma=gamma, weight=sr.WEIGHT)
    count = smooth.smoothness_count(d, image, order=order, space="inverse", depth=True)
    loss.backward()
    print(f"[smooth] {H}x{W} subnormal depth, infinite guide value, order {order} gamma {gamma}: loss {float(loss):.8f} want "
          f"{r['value']:.8f}; counted {int(count)}, reference {r['count']} ({plain['count']} without the two)")
    assert abs(float(loss) - r["value"]) <= max(rowbar.E32_MARGIN * abs(a["value"] - r["value"]), 1e-6)
    assert float(count) == r["count"]
    assert float(d.grad[4, 5]) == 0.0
    _gradient_bar(d.grad[None].cpu().numpy(), r["grad"], a["grad"], b["grad"], f"{H}x{W} subnormal depth, infinite guide, order {order}")


def test_a_single_channel_guide_is_the_three_channel_guide_of_equal_planes(hip_device):
    from luciddreamer_amd import smooth
    case = _case(67, 131, "smooth")
    d = torch.from_numpy(case["depth"]).to(hip_device)
    g1 = torch.from_numpy(case["guide"][:1]).to(hip_device)
    r = sr.reference(case["depth"][None], case["guide"][:1], order=2, positive_only=True)
    a = sr.restate32(case["depth"][None], case["guide"][:1], order=2, positive_only=True)
    loss = smooth.depth_smoothness(d, g1, order=2, gamma=sr.GAMMA, weight=sr.WEIGHT)
    print(f"[smooth] one-channel guide: loss {float(loss):.8f} want {r['value']:.8f}")
    assert abs(float(loss) - r["value"]) <= max(rowbar.E32_MARGIN * abs(a["value"] - r["value"]), 1e-6)
    assert float(smooth.smoothness_count(d, g1, order=2, depth=True)) == r["count"]


# ---- 2. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(67, 131), (600, 900)])
@pytest.mark.parametrize("order,space", [(1, "depth"), (2, "inverse")])
def test_repeated_calls_forms_upstream_and_gamma_zero(hip_device, H, W, order, space):
    case = _case(H, W, "smooth")
    first = _device(case, hip_device, "depth", order, space, True, upstream=1.3)
    again = _device(case, hip_device, "depth", order, space, True, upstream=1.3)
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]) and torch.equal(again[2], first[2])
    flat = _device(case, hip_device, "depth", order, space, True, upstream=1.3, flat=True)              # [H,W] input
    assert tuple(flat[2].shape) == (H, W) and tuple(first[2].shape) == (1, H, W)
    assert torch.equal(flat[0], first[0]) and torch.equal(flat[2], first[2][0])
    # the upstream scalars are honoured: 1.3 and -2.0 against the references evaluated with them
    for up, got in ((1.3, first), (-2.0, _device(case, hip_device, "depth", order, space, True, upstream=-2.0))):
        r, a, b = _refs(H, W, "smooth", "depth", order, space, True, up)
        _gradient_bar(got[2].cpu().numpy(), r["grad"], a["grad"], b["grad"], f"{H}x{W} order {order} {space} upstream {up}")
    # gamma = 0: every weight is expf(-0) = 1, the result without a guide, bit for bit
    zero = _device(case, hip_device, "depth", order, space, True, gamma=0.0)
    none = _device(case, hip_device, "depth", order, space, True, guide=None)
    assert torch.equal(zero[0], none[0]) and torch.equal(zero[1], none[1]) and torch.equal(zero[2], none[2])
    assert float(zero[0]) > float(_device(case, hip_device, "depth", order, space, True)[0]) > 0


# ---- 3. through the rasterizer ---------------------------------------------------------------------------------------------------
NAMES = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
RW, RH, RP = 64, 64, 400


@pytest.fixture
def depth_on():
    config.set_depth_gradient(True)
    yield
    config.set_depth_gradient(False)


@pytest.mark.parametrize("order,space", [(1, "depth"), (2, "inverse")])
def test_depth_smoothness_through_the_rasterizer(hip_device, depth_on, order, space):
    """depth_smoothness on the rasterizer's depth output: the value is the reference's on the rendered depth, and the gradient
    reaches the means and the opacities."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd import smooth
    cam, cloud = hp.box_setup(RP, RW, RH, scale_mult=2.0)
    tfx, tfy = hp.tan_fov(cam)
    c = cam.to(hip_device)
    rs = GaussianRasterizationSettings(cam.image_height, cam.image_width, tfx, tfy, torch.zeros(3, device=hip_device), 1.0,
                                       c.world_view_transform, c.full_proj_transform, 1, c.camera_center, False, False)
    leaves = {k: cloud[k].detach().to(hip_device).requires_grad_(True) for k in NAMES if k != "means2D"}
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
    out = GaussianRasterizer(rs)(**leaves)
    color, depth = out[0], out[2]
    assert tuple(depth.shape) == (1, RH, RW) and depth.requires_grad
    guide = color.detach()
    kw = dict(order=order, space=space, positive_only=True, gamma=sr.GAMMA, weight=sr.WEIGHT)
    r = sr.reference(depth.detach().cpu().numpy(), guide.cpu().numpy(), **kw)
    a = sr.restate32(depth.detach().cpu().numpy(), guide.cpu().numpy(), **kw)
    loss = smooth.depth_smoothness(depth, guide, order=order, space=space, gamma=sr.GAMMA, weight=sr.WEIGHT)
    print(f"[smooth] rasterizer {RH}x{RW}, {RP} Gaussians, order {order} {space}: {r['count']} terms counted, loss {float(loss):.6f} "
          f"want {r['value']:.6f}")
    assert r["count"] >= 0.25 * 2 * RH * RW and r["value"] > 0
    assert abs(float(loss.detach()) - r["value"]) <= max(rowbar.E32_MARGIN * abs(a["value"] - r["value"]), 1e-6)
    loss.backward()
    for k in ("means3D", "opacities"):
        g = leaves[k].grad
        print(f"[smooth] rasterizer {k}: max|g| {float(g.abs().max()):.3e}")
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    assert leaves["shs"].grad is None or not leaves["shs"].grad.any()      # the depth does not depend on the colours


# ---- 4. the example loop -----------------------------------------------------------------------------------------------------------
def test_example_loop_with_the_smoothness_term(hip_device):
    import importlib.util
    import math
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_loop_example_smooth_gpu", os.path.join(root, "examples", "train_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    plain, _ = mod.train(mod.default_args(gaussians=2000, iters=10, resolution="64x64", log=1), log=lambda s: None)
    losses, _ = mod.train(mod.default_args(gaussians=2000, iters=10, resolution="64x64", log=1, depth_smoothness=0.1,
                                           smoothness_order=2, smoothness_space="inverse"), log=lambda s: None)
    assert len(losses) == 10 and all(math.isfinite(l) for _, l, _ in losses)
    assert losses[0][1] > plain[0][1]                   # the term is in the loss from the first iteration on
    assert not config.depth_gradient()                  # the loop leaves the switch as it found it
