"""Median depth and per-pixel Gaussian ids on the GPU (return_median -> lr_render_median, lr_median_backward).

Parity with the numpy walk on the C oracle's state (tests/median_ref.py; its own properties: tests/test_median_cpu.py) under
default and strict evaluation, both forward shapes and both entry points; the invariants against the operator's own alpha output;
the gradient against the float64 reference built from the GPU's own ids, held to the float32 summation bound; the edges of the
C ABI; the video path.  Every test fails without the feature: return_median does not exist there."""
import ctypes

import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, config, synthetic
from tests import helpers as hp, median_ref as mr, posed_cases as pc_

pytestmark = pytest.mark.gpu

POSED = "box_general"                   # yaw, pitch, roll and a translation at once: all three components of the view's z row


@pytest.fixture
def exact_mode():
    """Bit comparisons between calls: every forward in exact mode (async mode's binning bound can pick another shape)."""
    config.set_async(False)
    yield
    config.set_async(True)
    config.reset()


def _settings(cam, bg, degree, dev):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings
    tfx, tfy = hp.tan_fov(cam)
    c = cam.to(dev)
    return GaussianRasterizationSettings(cam.image_height, cam.image_width, tfx, tfy, bg.to(dev), 1.0, c.world_view_transform,
                                         c.full_proj_transform, degree, c.camera_center, False, False)


NAMES = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")


def _run(cloud, cam, degree, bg, dev, median=True, alpha=False, gc=None, gm=None, fused=False):
    """GaussianRasterizer on fresh leaves; loss <gc, color> + <gm, median_depth> (terms left out when None)."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizer
    leaves = {k: cloud[k].detach().to(dev).requires_grad_(True) for k in NAMES if k != "means2D"}
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
    if fused:
        for t in leaves.values():
            t.grad = torch.zeros_like(t)
    kw = dict(return_alpha=True) if alpha else {}
    if median:
        kw["return_median"] = True
    config.set_fused_grad_accumulation(fused)
    try:
        out = GaussianRasterizer(_settings(cam, bg, degree, dev))(**leaves, **kw)
        res = dict(color=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy(), depth=out[2].detach().cpu().numpy())
        if alpha:
            res["alpha"] = out[3].detach().cpu().numpy()
        if median:
            assert not out[-1].requires_grad and out[-1].dtype == torch.int32
            res["median_depth"], res["median_ids"] = out[-2].detach().cpu().numpy(), out[-1].cpu().numpy()
        loss = None
        for t, g in ((out[0], gc), (out[-2] if median else None, gm)):
            if g is not None:
                term = (t * g.to(dev)).sum()
                loss = term if loss is None else loss + term
        if loss is not None:
            loss.backward()
            res["grads"] = {k: (np.zeros(tuple(t.shape), np.float32) if t.grad is None else t.grad.cpu().numpy())
                            for k, t in leaves.items()}
    finally:
        config.set_fused_grad_accumulation(False)
    return res


def _raw_cloud(cloud, degree, dev):
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    return GaussianCloud(cloud["means3D"].to(dev), cloud["scales"].to(dev), cloud["rotations"].to(dev), cloud["opacities"].to(dev),
                         cloud["shs"].to(dev), active_sh_degree=degree)


def _run_raw(cloud, cam, degree, bg, dev, gm=None):
    from luciddreamer_amd.gaussian_renderer import render_raw
    pc = _raw_cloud(cloud, degree, dev)
    out = render_raw(cam.to(dev), pc, bg_color=bg.to(dev), return_median=True)
    res = dict(median_depth=out["median_depth"].detach().cpu().numpy(), median_ids=out["median_ids"].cpu().numpy())
    if gm is not None:
        (out["median_depth"] * gm.to(dev)).sum().backward()
        res["xyz_grad"] = pc._xyz.grad.cpu().numpy()
    return res


def _G(H, W, seed=31):
    """Seeded upstream of the median depth, |G| in [0.5, 1.5) with random signs: no pixel's weight is lost against another's."""
    g = torch.Generator().manual_seed(seed)
    return ((0.5 + torch.rand(1, H, W, generator=g)) * (1.0 - 2.0 * torch.randint(0, 2, (1, H, W), generator=g))).float()


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("name", mr.PARITY_INPUTS)
def test_parity_with_the_reference_walk(hip_device, exact_mode, name, strict):
    cam, cloud = mr.box_input(name)
    r = mr.box_reference(name)
    bg = torch.tensor(mr.BG)
    n_pix = r["ids"].size
    assert r["fragile"].sum() <= mr.FRAGILE_CAP * n_pix
    config.set_strict_parity(strict)
    outs = {}
    try:
        for shape in (0, 2):
            _lib.tune_set("fwd_pair", shape)
            outs[("activated", shape)] = _run(cloud, cam, mr.DEGREE, bg, hip_device)
            assert _lib.last_launch_shapes()[0] == ("quadrant", None, "tile")[shape]
            outs[("raw", shape)] = _run_raw(cloud, cam, mr.DEGREE, bg, hip_device)
    finally:
        _lib.tune_set("fwd_pair", -1)
        config.set_strict_parity(False)
    for key, o in outs.items():
        ids, depth = o["median_ids"], o["median_depth"][0]
        differ = ids != r["ids"]
        print(name, "strict" if strict else "default", key, "differing", int(differ.sum()), "fragile", int(r["fragile"].sum()))
        assert not (differ & ~r["fragile"]).any(), key                  # equal on every non-fragile pixel ...
        assert differ.sum() <= mr.FRAGILE_CAP * n_pix, key               # ... and the differing ones are few
        # the depth of the GPU's own choice: the oracle's per-Gaussian depth
        has = ids >= 0
        want = r["st"]["depths"][ids[has]]
        assert (np.abs(depth[has] - want) <= hp.DEPTH_RTOL * np.maximum(1.0, np.abs(want))).all(), key
        assert not depth[~has].any() and (ids[~has] == -1).all(), key
    first = outs[("activated", 0)]
    for key, o in outs.items():                                         # one parity mode: the same bits from all four
        assert np.array_equal(o["median_ids"], first["median_ids"]), key
        assert np.array_equal(o["median_depth"].view(np.uint32), first["median_depth"].view(np.uint32)), key


# ---- 2. invariants ------------------------------------------------------------------------------------------------------------
WIDE = (1000, 150, 110, 4.0)            # P, W, H, scale_mult: footprints on both sides of the backward's one-wave limit


def _box_pixels(st, radii, W, H):
    """Pixels of the box the backward scans per Gaussian (render_median.hip med_box), restated on the oracle's state: the tile
    rectangle (the reference's getRect), clipped to the image, cut down to the bounding box of the alpha >= 1/255 ellipse
    0.5 (a dx^2 + c dy^2) + b dx dy <= log(255 opacity) + 0.02, one pixel wider."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    x, y, r = st["means2D"][:, 0].astype(np.float64), st["means2D"][:, 1].astype(np.float64), radii.astype(np.float64)
    a, b, c, op = (st["conic_opacity"][:, i].astype(np.float64) for i in range(4))
    lo = lambda m, g: np.clip(((m - r) / 16).astype(np.int64), 0, g)
    hi = lambda m, g: np.clip(((m + r + 15) / 16).astype(np.int64), 0, g)
    with np.errstate(all="ignore"):
        k = 2.0 * (np.log(255.0 * op) + 0.02) / (a * c - b * b)
        hx, hy = np.sqrt(k * c) + 1.0, np.sqrt(k * a) + 1.0
    x0, x1 = np.maximum(lo(x, gx) * 16, np.ceil(x - hx)), np.minimum(np.minimum(W, hi(x, gx) * 16), np.floor(x + hx) + 1)
    y0, y1 = np.maximum(lo(y, gy) * 16, np.ceil(y - hy)), np.minimum(np.minimum(H, hi(y, gy) * 16), np.floor(y + hy) + 1)
    return np.where(radii > 0, np.maximum(x1 - x0, 0) * np.maximum(y1 - y0, 0), 0)


def _invariant_case(name):
    if name == "wide":
        P, W, H, s = WIDE
        cam, cloud = hp.box_setup(P, W, H, seed=0, scale_mult=s)
        return cam, cloud, mr.DEGREE, torch.tensor(mr.BG)
    if name == "posed":
        cam, cloud, degree = pc_.make(POSED)
        return cam, cloud, degree, torch.tensor(pc_.BG)
    cam, cloud = mr.box_input(name)
    return cam, cloud, mr.DEGREE, torch.tensor(mr.BG)


@pytest.mark.parametrize("name", sorted(mr.INPUTS) + ["posed"])
def test_invariants_against_the_alpha_output(hip_device, exact_mode, name):
    cam, cloud, degree, bg = _invariant_case(name)
    gc = synthetic.upstream_grad(cam.image_height, cam.image_width)
    o = _run(cloud, cam, degree, bg, hip_device, alpha=True, gc=gc)
    ids, depth, alpha = o["median_ids"], o["median_depth"][0], o["alpha"][0]
    assert (ids[alpha > 0.5] >= 0).all()
    below = alpha < 0.5                                                 # (alpha == 0.5 is free: 1 - T rounds there)
    assert (ids[below] == -1).all() and not depth[below].any()
    has = ids >= 0
    assert has.any() and ids.max() < cloud["means3D"].shape[0]
    assert (o["radii"][ids[has]] > 0).all()
    assert (depth[has] > 0.2).all()                                     # in front of the near plane
    # unused median outputs: everything else is what the call without them gives, to the bit
    plain = _run(cloud, cam, degree, bg, hip_device, median=False, alpha=True, gc=gc)
    for k in ("color", "depth", "radii", "alpha"):
        assert np.array_equal(o[k], plain[k]), k
    for k in NAMES:
        assert np.array_equal(o["grads"][k], plain["grads"][k]), k


# ---- 3. gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "posed", "wide"])
def test_gradient_reaches_means3D_through_the_view_row(hip_device, exact_mode, name):
    """means3D.grad of <G, median_depth> (+ a colour loss) minus the colour-only gradient against the float64 reference built from
    the GPU's own ids.  Per row the tolerance is (n_g + 2) 2^-24 sum_p |G[p]| max|view row|: the float32 bound of a sum of n_g
    terms in any order, one rounding of the product with the view row, one of the addition to the colour gradient -- which holds
    as long as the colour gradient the term is added to does not exceed the term's own scale, hence the small colour upstream
    (asserted below).  Nothing fitted."""
    cam, cloud, degree, bg = _invariant_case(name)
    H, W = cam.image_height, cam.image_width
    P = cloud["means3D"].shape[0]
    G = _G(H, W)
    gc = 1e-3 * synthetic.upstream_grad(H, W)
    view = cam.world_view_transform.numpy().reshape(-1)
    vmax = float(np.abs(view[[2, 6, 10]]).max())
    if name == "posed":
        assert (np.abs(view[[2, 6, 10]]) > 0.05).all()                  # all three components are exercised

    alone = _run(cloud, cam, degree, bg, hip_device, gm=G)
    colour = _run(cloud, cam, degree, bg, hip_device, gc=gc)
    both = _run(cloud, cam, degree, bg, hip_device, gc=gc, gm=G)
    ids = both["median_ids"]
    assert np.array_equal(ids, alone["median_ids"])
    ref, n, sabs = mr.grad_means3D(ids, G.numpy(), view, P)
    tol = (n + 2) * 2.0 ** -24 * sabs * vmax
    owns = n > 0
    assert owns.sum() > 50 and n.max() > 8
    if name == "wide":
        # the backward sums rectangles of up to 64 x 64 pixels with one wave and larger ones with a workgroup: both are met
        o = hp.run_oracle(cloud, cam, degree, bg)
        box = _box_pixels(o["res"].stage(), o["radii"], W, H)
        assert (box[owns] > 64 * 64 + 200).sum() >= 10 and (box[owns] < 64 * 64 - 200).sum() > 10
        assert n[box > 64 * 64 + 200].max() > 64 and (n[owns] <= box[owns]).all()
    assert float(np.abs(colour["grads"]["means3D"][owns]).max()) <= 0.5 * vmax      # the premise of the bound (docstring)

    for run, base in ((alone, np.zeros((P, 3))), (both, colour["grads"]["means3D"].astype(np.float64))):
        term = run["grads"]["means3D"].astype(np.float64) - base
        err = np.abs(term - ref).max(axis=1)
        worst = int(np.argmax(np.where(owns, err / np.maximum(tol, 1e-300), 0.0)))
        print(name, "worst row", worst, "err", err[worst], "tol", tol[worst], "n", int(n[worst]))
        assert (err <= tol).all(), (worst, err[worst], tol[worst])
        # rows that own no pixel: exactly the colour-only value
        assert np.array_equal(run["grads"]["means3D"][~owns], base[~owns].astype(np.float32))
    # nothing flows anywhere else: every other gradient of the median-only loss is zero, and with the colour loss the colour's
    for k in NAMES:
        if k != "means3D":
            assert not alone["grads"][k].any(), k
            assert np.array_equal(both["grads"][k], colour["grads"][k]), k

    # fused gradient accumulation on: the same bits
    fused = _run(cloud, cam, degree, bg, hip_device, gc=gc, gm=G, fused=True)
    assert np.array_equal(fused["grads"]["means3D"], both["grads"]["means3D"])
    # two runs: bit-identical, forward and backward
    again = _run(cloud, cam, degree, bg, hip_device, gc=gc, gm=G)
    assert np.array_equal(again["median_ids"], ids)
    assert np.array_equal(again["median_depth"].view(np.uint32), both["median_depth"].view(np.uint32))
    assert np.array_equal(again["grads"]["means3D"].view(np.uint32), both["grads"]["means3D"].view(np.uint32))

    # the raw entry point: xyz.grad of the median-only loss is the same sum
    raw = _run_raw(cloud, cam, degree, bg, hip_device, gm=G)
    ref_raw, n_raw, sabs_raw = mr.grad_means3D(raw["median_ids"], G.numpy(), view, P)
    assert (np.abs(raw["xyz_grad"].astype(np.float64) - ref_raw).max(axis=1) <= (n_raw + 2) * 2.0 ** -24 * sabs_raw * vmax).all()


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------
def _forward_c_abi(cloud, cam, dev, capacity):
    from luciddreamer_amd import _C
    tfx, tfy = hp.tan_fov(cam)
    camd = cam.to(dev)
    return _C.rasterize_gaussians(torch.zeros(3, device=dev), cloud["means3D"].to(dev), torch.Tensor([]),
                                  cloud["opacities"].to(dev), cloud["scales"].to(dev), cloud["rotations"].to(dev), 1.0,
                                  torch.Tensor([]), camd.world_view_transform, camd.full_proj_transform, tfx, tfy,
                                  cam.image_height, cam.image_width, cloud["shs"].to(dev), 3, camd.camera_center, False, False,
                                  binning_capacity=capacity)


def test_empty_cloud_and_cloud_behind_the_camera(hip_device, exact_mode):
    cam, cloud = mr.box_input("small")
    bg = torch.tensor(mr.BG)
    empty = {k: v[:0].contiguous() for k, v in cloud.items()}
    o = _run(empty, cam, mr.DEGREE, bg, hip_device)
    assert (o["median_ids"] == -1).all() and not o["median_depth"].any()
    behind = dict(cloud, means3D=(cloud["means3D"] * torch.tensor([1.0, 1.0, -1.0])).contiguous())
    o = _run(behind, cam, mr.DEGREE, bg, hip_device, gm=_G(cam.image_height, cam.image_width))
    assert (o["median_ids"] == -1).all() and not o["median_depth"].any()
    assert not o["grads"]["means3D"].any()


def test_median_of_an_async_rerender_is_the_rerenders(hip_device):
    """Async mode with the verify policy and a binning buffer far too small: the view is rendered again, and the median outputs
    and their gradient come from the returned forward's buffers -- equal to an exact-mode render's."""
    cam, cloud = mr.box_input("sparse")
    bg = torch.tensor(mr.BG)
    G = _G(cam.image_height, cam.image_width)
    config.set_async(False)
    try:
        exact = _run(cloud, cam, mr.DEGREE, bg, hip_device, gm=G)
    finally:
        config.set_async(True)
        config.reset()
    config.set_async(True, headroom=1.0, warm_calls=1)
    try:
        with torch.no_grad():
            _run(cloud, cam, mr.DEGREE, bg, hip_device)
        key = next(iter(config._hwm))
        config._hwm[key] = 64                                # the next forward overflows and is rendered again
        got = _run(cloud, cam, mr.DEGREE, bg, hip_device, gm=G)
    finally:
        config.reset()
        config.set_async(True)
    assert (exact["median_ids"] >= 0).any()
    assert np.array_equal(got["median_ids"], exact["median_ids"]) and np.array_equal(got["median_depth"], exact["median_depth"])
    assert np.array_equal(got["grads"]["means3D"], exact["grads"]["means3D"])


def test_c_abi_overflow_null_ids_and_struct_bytes(hip_device):
    from luciddreamer_amd import _C
    cam, cloud = mr.box_input("sparse")
    H, W, P = cam.image_height, cam.image_width, cloud["means3D"].shape[0]
    # an async forward whose binning capacity is too small: 0 / -1 everywhere, rc 0, the overflow is lr_check's to report
    out = _forward_c_abi(cloud, cam, hip_device, 100)
    depth, ids = _C.render_median(out[4], out[5], out[6], P, H, W, binning_capacity=100)
    assert (ids == -1).all() and not depth.any()
    with pytest.raises(RuntimeError, match="capacity"):
        _C.check(out[4])
    g = _C.median_backward(out[4], out[5], out[6], out[3], ids, torch.ones(1, H, W, device=hip_device),
                           cam.to(hip_device).world_view_transform, binning_capacity=100)
    assert not g.any()
    # a capacity that holds the view: the exact forward's outputs; out_ids = NULL leaves the depth as it is
    exact = _forward_c_abi(cloud, cam, hip_device, 0)
    d0, i0 = _C.render_median(exact[4], exact[5], exact[6], P, H, W)
    roomy = _forward_c_abi(cloud, cam, hip_device, 4 * int(exact[0]) + 1024)
    d1, i1 = _C.render_median(roomy[4], roomy[5], roomy[6], P, H, W, binning_capacity=4 * int(exact[0]) + 1024)
    assert torch.equal(i0, i1) and torch.equal(d0, d1) and (i0 >= 0).any()
    d2, none = _C.render_median(exact[4], exact[5], exact[6], P, H, W, want_ids=False)
    assert none is None and torch.equal(d2, d0)
    # a wrong struct_bytes, with everything else in place
    L = _lib.lib()
    a = _lib.MedianArgs(geom_buffer=exact[4].data_ptr(), binning_buffer=exact[5].data_ptr(), image_buffer=exact[6].data_ptr(), P=P,
                        width=W, height=H, out_median_depth=d0.data_ptr(), out_ids=i0.data_ptr(),
                        stream=torch.cuda.current_stream(hip_device).cuda_stream)
    a.struct_bytes = ctypes.sizeof(_lib.MedianArgs) - 8
    assert L.lr_render_median(a) == _lib.LR_ERR_INVALID_ARG
    b = _lib.MedianBackwardArgs()
    b.struct_bytes += 8
    assert L.lr_median_backward(b) == _lib.LR_ERR_INVALID_ARG
    torch.cuda.synchronize()


def test_render_only_and_install_pass_median_through(hip_device):
    from types import SimpleNamespace
    from luciddreamer_amd import cameras, dropin
    from luciddreamer_amd.gaussian_renderer import render, render_raw
    W, H = 128, 96
    pc = _raw_cloud(synthetic.make_cloud(5_000, "band", 4), 1, hip_device)
    cam = cameras.rotate360_path(W, H, n_views=12)[0].to(hip_device)
    b = render_raw(cam, pc, render_only=True, return_median=True)
    assert set(b) == {"render", "depth", "median_depth", "median_ids"} and "median_depth" not in render(cam, pc)
    both = render(cam, pc, return_alpha=True, return_median=True)
    assert torch.equal(both["median_ids"], b["median_ids"]) and both["alpha"].shape == (1, H, W) and (b["median_ids"] >= 0).any()

    def reference_render(*args, **kw):
        raise AssertionError("the reference's render cannot return the median depth")
    ns = SimpleNamespace(render=reference_render)
    opt = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    h = dropin.install(ns, None, None, losses=False, adam=False, stats=False)
    try:
        out = ns.render(cam, pc, opt, torch.zeros(3, device=hip_device), return_median=True)
        over = ns.render(cam, pc, opt, torch.zeros(3, device=hip_device), override_color=torch.ones_like(pc._xyz),
                         return_median=True)
    finally:
        dropin.uninstall(h)
    assert torch.equal(out["median_ids"], b["median_ids"]) and torch.equal(out["median_depth"], b["median_depth"])
    assert torch.equal(over["median_ids"], b["median_ids"])


def test_armed_fused_step_takes_the_median_gradient(hip_device):
    """The armed FusedAdam (raw node's no-zero-fill backward + masked step) with a colour + median-depth loss: the same parameter
    bits as backward + step()."""
    import torch.nn as nn
    from luciddreamer_amd import cameras
    from luciddreamer_amd.gaussian_renderer import render_raw
    from tests.test_gpu_optim import _adam_for, _two_clouds
    params = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    W, H = 320, 192
    a, b = _two_clouds(40_000, hip_device)
    for cl in (a, b):
        for n in params:
            setattr(cl, n, nn.Parameter(getattr(cl, n).detach()))
    opt_a, opt_b = _adam_for(a), _adam_for(b)
    cams = [c.to(hip_device) for c in cameras.rotate360_path(W, H, n_views=12)]
    bg = torch.zeros(3, device=hip_device)
    gen = torch.Generator().manual_seed(13)
    for it in range(3):
        cam = cams[(5 * it) % 12]
        g = torch.randn(3, H, W, generator=gen).to(hip_device)
        gm = torch.randn(1, H, W, generator=gen).to(hip_device)
        pa = render_raw(cam, a, bg_color=bg, return_median=True)
        ((pa["render"] * g).sum() + (pa["median_depth"] * gm).sum()).backward()
        opt_a.step()
        opt_a.zero_grad(set_to_none=True)
        assert opt_b.arm_fused_backward()
        pb = render_raw(cam, b, bg_color=bg, return_median=True)
        ((pb["render"] * g).sum() + (pb["median_depth"] * gm).sum()).backward()
        assert all(getattr(b, n).grad is None for n in params)
        opt_b.step()
        opt_b.zero_grad(set_to_none=True)
        assert (pa["median_ids"] >= 0).any() and torch.equal(pa["median_ids"], pb["median_ids"]), it
        for n in params:
            assert torch.equal(getattr(a, n), getattr(b, n)), (it, n)


# ---- 5. video -----------------------------------------------------------------------------------------------------------------
def test_video_frames_of_the_median_depth(hip_device):
    from luciddreamer_amd import cameras
    from luciddreamer_amd.gaussian_renderer import render
    from luciddreamer_amd.video import colorize_depth, render_video_frames
    W, H = 64, 48
    pc = _raw_cloud(synthetic.make_cloud(20_000, "band", 0), 3, hip_device)
    views = [v.to(hip_device) for v in cameras.rotate360_path(W, H, n_views=3)]
    bg = torch.tensor([0.1, 0.2, 0.3], device=hip_device)
    frames, depths = render_video_frames(views, pc, None, bg, depth="median")
    plain_frames, plain_depths = render_video_frames(views, pc, None, bg)
    assert len(frames) == len(depths) == 3
    differs = False
    for i, v in enumerate(views):
        with torch.no_grad():
            out = render(v, pc, None, bg, return_median=True)
        want = colorize_depth(out["median_depth"])[0].cpu().numpy()
        assert depths[i].dtype == np.uint8 and np.array_equal(depths[i], want), i
        assert np.array_equal(frames[i], plain_frames[i]), i
        differs |= not np.array_equal(depths[i], plain_depths[i])
    assert differs                                                      # not the expected depth under another name
    with pytest.raises(ValueError):
        render_video_frames(views, pc, None, bg, depth="mean")
