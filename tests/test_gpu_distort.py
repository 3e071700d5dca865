"""Depth distortion on the GPU (return_distortion -> lr_render_distortion, lr_distortion_backward).

The forward against the float64 reference (tests/distort_ref.py; its own properties and the measured float32 error the bar comes
from: tests/test_distort_cpu.py) under default and strict evaluation, both forward shapes and both entry points; the shift
through the C ABI; every leaf's gradient against float64 autograd at GRAD_RTOL; how the term composes with the colour backward,
fused accumulation and the armed optimizer step; anti-aliasing; the edges of the C ABI.  Every test fails without the feature:
return_distortion and the entry points do not exist there."""
import ctypes

import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, config, synthetic
from tests import distort_ref as dr, helpers as hp

pytestmark = pytest.mark.gpu

NAMES = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
REF_KEY = dict(means3D="means3D", means2D="means2D", opacities="opacity", shs="sh", scales="scales", rotations="rotations")
RAW = (("xyz", "_xyz"), ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"))
FWD_BAR = 4.0                           # x distort_ref.FWD_ERR (its comment)


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


def _run(cloud, cam, degree, bg, dev, mapping="ndc", gc=None, gd=None, distortion=True, alpha=False, median=False, fused=False):
    """GaussianRasterizer on fresh leaves; loss <gc, color> + <gd, distortion> (terms left out when None)."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizer
    leaves = {k: cloud[k].detach().to(dev).requires_grad_(True) for k in NAMES if k != "means2D"}
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
    if fused:
        for t in leaves.values():
            t.grad = torch.zeros_like(t)
    kw = {}
    if alpha:
        kw["return_alpha"] = True
    if median:
        kw["return_median"] = True
    if distortion:
        kw.update(return_distortion=True, distortion_map=mapping)
    config.set_fused_grad_accumulation(fused)
    try:
        out = GaussianRasterizer(_settings(cam, bg, degree, dev))(**leaves, **kw)
        assert len(out) == 3 + bool(alpha) + 2 * bool(median) + bool(distortion)
        res = dict(color=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy(), depth=out[2].detach().cpu().numpy())
        if alpha:
            res["alpha"] = out[3].detach().cpu().numpy()
        if median:
            k = 3 + bool(alpha)
            assert out[k + 1].dtype == torch.int32
            res["median_depth"], res["median_ids"] = out[k].detach().cpu().numpy(), out[k + 1].cpu().numpy()
        if distortion:
            assert out[-1].shape == (1, cam.image_height, cam.image_width) and out[-1].dtype == torch.float32
            res["distortion"] = out[-1].detach().cpu().numpy()
        loss = None
        for t, g in ((out[0], gc), (out[-1] if distortion else None, gd)):
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


def _run_raw(cloud, cam, degree, bg, dev, mapping="ndc", gd=None):
    from luciddreamer_amd.gaussian_renderer import render_raw
    pc = _raw_cloud(cloud, degree, dev)
    out = render_raw(cam.to(dev), pc, bg_color=bg.to(dev), return_distortion=True, distortion_map=mapping)
    res = dict(distortion=out["distortion"].detach().cpu().numpy())
    if gd is not None:
        (out["distortion"] * gd.to(dev)).sum().backward()
        res["grads"] = {k: getattr(pc, a).grad.cpu().numpy() for k, a in RAW}
        res["grads"]["means2D"] = out["viewspace_points"].grad.cpu().numpy()
        res["grads"]["features_dc"] = pc._features_dc.grad.cpu().numpy()
        res["grads"]["features_rest"] = pc._features_rest.grad.cpu().numpy()
    return res


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. forward parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("mapping", sorted(dr.MAPS))
@pytest.mark.parametrize("name", sorted(dr.INPUTS) + ["posed"])
def test_forward_parity_with_the_float64_reference(hip_device, exact_mode, name, mapping, strict):
    """Every non-fragile pixel within 4 x the float32 walk's own measured error; D >= 0; exact zeros below two layers.  The two
    forward shapes leave the same bits behind each entry point.  (The raw entry point is fed log / logit of the parameters and takes
    exp / sigmoid of them in its kernels: its records are not the activated call's bits, so the two entry points are compared
    through the reference, each within the bar, and by bits only where the inputs are the same bits.)"""
    cam, cloud, degree, bg = dr.case(name)
    r = dr.reference(name, mapping)
    ok = ~r["fragile"]
    assert r["fragile"].sum() <= dr.FRAGILE_CAP * r["fragile"].size
    bar = FWD_BAR * dr.FWD_ERR[(name, mapping)]
    config.set_strict_parity(strict)
    outs = {}
    try:
        for shape in (0, 2):
            _lib.tune_set("fwd_pair", shape)
            outs[("activated", shape)] = _run(cloud, cam, degree, bg, hip_device, mapping)["distortion"][0]
            assert _lib.last_launch_shapes()[0] == ("quadrant", None, "tile")[shape]
            outs[("raw", shape)] = _run_raw(cloud, cam, degree, bg, hip_device, mapping)["distortion"][0]
    finally:
        _lib.tune_set("fwd_pair", -1)
        config.set_strict_parity(False)
    for key, D in outs.items():
        err = float(np.abs(D.astype(np.float64) - r["D64"])[ok].max())
        print(name, mapping, "strict" if strict else "default", key, "err %.3e" % err, "bar %.3e" % bar, "D max %.3e" % r["D64"].max())
    print("raw against activated: %d pixels differ in bits, by %.3e at most" % (
        int((_bits(outs[("raw", 0)]) != _bits(outs[("activated", 0)])).sum()), float(np.abs(outs[("raw", 0)] - outs[("activated", 0)]).max())))
    for key, D in outs.items():
        err = float(np.abs(D.astype(np.float64) - r["D64"])[ok].max())
        assert err <= bar, (key, err, bar)
        assert (D >= 0).all(), key
        assert not D[ok & (r["layers64"] < 2)].any(), key
        assert D[ok & (r["layers64"] >= 2)].any(), key
    for entry in ("activated", "raw"):
        assert np.array_equal(_bits(outs[(entry, 0)]), _bits(outs[(entry, 2)])), entry


# ---- 2. shift -----------------------------------------------------------------------------------------------------------------
def _forward_c_abi(cloud, cam, dev, capacity):
    from luciddreamer_amd import _C
    tfx, tfy = hp.tan_fov(cam)
    camd = cam.to(dev)
    return _C.rasterize_gaussians(torch.zeros(3, device=dev), cloud["means3D"].to(dev), torch.Tensor([]),
                                  cloud["opacities"].to(dev), cloud["scales"].to(dev), cloud["rotations"].to(dev), 1.0,
                                  torch.Tensor([]), camd.world_view_transform, camd.full_proj_transform, tfx, tfy,
                                  cam.image_height, cam.image_width, cloud["shs"].to(dev), 3, camd.camera_center, False, False,
                                  binning_capacity=capacity)


def test_shift_through_the_c_abi(hip_device):
    """Linear mapping with c0 = 0 against c0 = 1000: within 4 x the float32 walk's own difference for the pair."""
    from luciddreamer_amd import _C
    cam, cloud, _, _ = dr.case("sparse")
    H, W, P = cam.image_height, cam.image_width, cloud["means3D"].shape[0]
    f = _forward_c_abi(cloud, cam, hip_device, 0)
    a, ma = _C.render_distortion(f[4], f[5], f[6], P, H, W, distortion_map=dr.SHIFT_PAIR[0])
    b, mb = _C.render_distortion(f[4], f[5], f[6], P, H, W, distortion_map=dr.SHIFT_PAIR[1])
    err = float((a - b).abs().max())
    print("shift pair: max difference %.3e" % err, "bar %.3e" % (4 * dr.SHIFT_ERR), "D max %.3e" % float(a.max()))
    assert float(a.max()) > 0.5 and err <= 4 * dr.SHIFT_ERR
    has = ma[..., 0] > 0                                    # the reference depth is the first layer's mapped depth
    assert torch.allclose(mb[..., 3][has] - ma[..., 3][has], torch.full_like(ma[..., 3][has], 1000.0), rtol=0, atol=1e-3)


# ---- 3. backward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("mapping", sorted(dr.MAPS))
@pytest.mark.parametrize("name", ["sparse", "dense", "wide", "posed"])
def test_gradients_against_float64_autograd(hip_device, exact_mode, name, mapping, strict):
    """Every leaf of both entry points at GRAD_RTOL for a seeded upstream that is zero on the fragile pixels (on both sides);
    colour and SH gradients are exact zeros when only D carries a gradient."""
    cam, cloud, degree, bg = dr.case(name)
    r = dr.reference(name, mapping)
    config.set_strict_parity(strict)
    try:
        act = _run(cloud, cam, degree, bg, hip_device, mapping, gd=r["G"])
        raw = _run_raw(cloud, cam, degree, bg, hip_device, mapping, gd=r["G"])
    finally:
        config.set_strict_parity(False)
    got = {REF_KEY[k]: v for k, v in act["grads"].items()}
    names = ["means3D", "means2D", "opacity", "scales", "rotations"]
    for k in names:
        ref = r["leaf"][k]
        print(name, mapping, k, "err %.2e of max |g| = %.3e" % (np.abs(got[k].reshape(ref.shape) - ref).max() / np.abs(ref).max(),
                                                                np.abs(ref).max()))
    hp.compare_grads(got, r["leaf"], names=names)
    assert not act["grads"]["shs"].any()
    want = dr.raw_grads(cloud, r["leaf"])
    for k in want:
        print(name, mapping, "raw", k, "err %.2e" % (np.abs(raw["grads"][k].reshape(want[k].shape) - want[k]).max() / np.abs(want[k]).max()))
    hp.compare_grads(raw["grads"], want, names=list(want))
    assert not raw["grads"]["features_dc"].any() and not raw["grads"]["features_rest"].any()


# ---- 4. composition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "posed"])
def test_composition_with_the_colour_backward(hip_device, exact_mode, name):
    cam, cloud, degree, bg = dr.case(name)
    H, W = cam.image_height, cam.image_width
    r = dr.reference(name, "ndc")
    # the distortion of the "ndc" mapping is small: an upstream that brings its gradient to the colour gradient's size
    gd = r["G"] * 1000.0
    gc = synthetic.upstream_grad(H, W)
    colour = _run(cloud, cam, degree, bg, hip_device, gc=gc, distortion=False)
    alone = _run(cloud, cam, degree, bg, hip_device, gd=gd)
    both = _run(cloud, cam, degree, bg, hip_device, gc=gc, gd=gd)
    for k in NAMES:
        c, d, b = (x["grads"][k].astype(np.float64) for x in (colour, alone, both))
        scale = max(np.abs(c).max(), np.abs(d).max())
        print(name, k, "colour max %.3e distortion max %.3e" % (np.abs(c).max(), np.abs(d).max()), "err %.2e" % (np.abs(b - (c + d)).max() / scale))
        assert np.abs(b - (c + d)).max() <= hp.GRAD_RTOL * scale, k
        if k != "shs":
            assert np.abs(d).max() > 0.01 * np.abs(c).max(), k       # the term is not lost against the colour's
    # fused gradient accumulation on: the same bits; two runs: the same bits, forward and backward
    fused = _run(cloud, cam, degree, bg, hip_device, gc=gc, gd=gd, fused=True)
    again = _run(cloud, cam, degree, bg, hip_device, gc=gc, gd=gd)
    assert np.array_equal(_bits(again["distortion"]), _bits(both["distortion"]))
    for k in NAMES:
        # (values, as tests/test_gpu_median.py compares them: a row that is -0 when written is +0 when added to a zeroed .grad)
        differ = fused["grads"][k] != both["grads"][k]
        print(name, k, "fused against unfused:", int(differ.sum()), "values differ, by",
              float(np.abs(fused["grads"][k] - both["grads"][k]).max()), "at most")
        assert np.array_equal(fused["grads"][k], both["grads"][k]), k
        assert np.array_equal(_bits(again["grads"][k]), _bits(both["grads"][k])), k
    # an unused distortion output (with unused alpha and median outputs next to it): the colour gradients' bits
    unused = _run(cloud, cam, degree, bg, hip_device, gc=gc, alpha=True, median=True)
    for k in ("color", "depth", "radii"):
        assert np.array_equal(unused[k], colour[k]), k
    for k in NAMES:
        assert np.array_equal(_bits(unused["grads"][k]), _bits(colour["grads"][k])), k
    # all three requested: each output is what it is when requested alone
    assert np.array_equal(_bits(unused["distortion"]), _bits(both["distortion"]))
    a = _run(cloud, cam, degree, bg, hip_device, distortion=False, alpha=True)
    m = _run(cloud, cam, degree, bg, hip_device, distortion=False, median=True)
    assert np.array_equal(_bits(unused["alpha"]), _bits(a["alpha"]))
    assert np.array_equal(unused["median_ids"], m["median_ids"]) and np.array_equal(_bits(unused["median_depth"]), _bits(m["median_depth"]))


def test_armed_fused_step_takes_the_distortion_gradient(hip_device):
    """The armed FusedAdam (raw node's no-zero-fill backward + masked step) with a colour + distortion loss: the same parameter
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
    moved = False
    for it in range(3):
        cam = cams[(5 * it) % 12]
        g = torch.randn(3, H, W, generator=gen).to(hip_device)
        gd = (1000.0 * torch.randn(1, H, W, generator=gen)).to(hip_device)
        pa = render_raw(cam, a, bg_color=bg, return_distortion=True)
        ((pa["render"] * g).sum() + (pa["distortion"] * gd).sum()).backward()
        opt_a.step()
        opt_a.zero_grad(set_to_none=True)
        assert opt_b.arm_fused_backward()
        pb = render_raw(cam, b, bg_color=bg, return_distortion=True)
        ((pb["render"] * g).sum() + (pb["distortion"] * gd).sum()).backward()
        assert all(getattr(b, n).grad is None for n in params)
        opt_b.step()
        opt_b.zero_grad(set_to_none=True)
        moved |= bool((pa["distortion"] > 0).any())
        assert torch.equal(pa["distortion"], pb["distortion"]), it
        for n in params:
            assert torch.equal(getattr(a, n), getattr(b, n)), (it, n)
    assert moved


# ---- 5. anti-aliasing ---------------------------------------------------------------------------------------------------------
def test_gradients_with_antialiasing_on(hip_device, exact_mode):
    """The blend sees opacity x coef (tests/aa_ref.py): the reference is fed the compensated opacity, whose own derivative reaches
    the scales."""
    cam, cloud, degree, bg = dr.case("sparse")
    r = dr.aa_reference("sparse", "linear")
    plain = dr.reference("sparse", "linear")
    assert np.abs(r["leaf"]["scales"] - plain["leaf"]["scales"]).max() > 100 * hp.GRAD_RTOL * np.abs(plain["leaf"]["scales"]).max()
    config.set_antialiasing(True)
    try:
        got = _run(cloud, cam, degree, bg, hip_device, "linear", gd=r["G"])
    finally:
        config.set_antialiasing(False)
    ok = ~r["fragile"]
    assert np.abs(got["distortion"][0].astype(np.float64) - r["D64"])[ok].max() <= FWD_BAR * dr.FWD_ERR[("sparse", "linear")]
    hp.compare_grads(dict(opacity=got["grads"]["opacities"], scales=got["grads"]["scales"]), r["leaf"], names=["opacity", "scales"])


# ---- 6. edges of the C ABI ----------------------------------------------------------------------------------------------------
def test_c_abi_edges(hip_device):
    from luciddreamer_amd import _C
    cam, cloud, _, _ = dr.case("sparse")
    H, W, P = cam.image_height, cam.image_width, cloud["means3D"].shape[0]
    dev = hip_device
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rs = _settings(cam, torch.zeros(3), 3, dev)
    inputs = dict(means3D=cloud["means3D"].to(dev), scales=cloud["scales"].to(dev), rotations=cloud["rotations"].to(dev))
    exact = _forward_c_abi(cloud, cam, dev, 0)
    d0, m0 = _C.render_distortion(exact[4], exact[5], exact[6], P, H, W)
    assert (d0 > 0).any() and m0.shape == (H, W, 4)
    # a capacity that holds the view: the exact forward's outputs
    roomy = _forward_c_abi(cloud, cam, dev, 4 * int(exact[0]) + 1024)
    d1, m1 = _C.render_distortion(roomy[4], roomy[5], roomy[6], P, H, W, binning_capacity=4 * int(exact[0]) + 1024)
    assert torch.equal(d0, d1) and torch.equal(m0, m1)
    # an async forward whose binning capacity is too small: zeros, rc 0, the overflow is lr_check's to report; the backward adds nothing
    over = _forward_c_abi(cloud, cam, dev, 100)
    d, m = _C.render_distortion(over[4], over[5], over[6], P, H, W, binning_capacity=100)
    assert not d.any() and not m.any()
    with pytest.raises(RuntimeError, match="capacity"):
        _C.check(over[4])
    acc = {k: torch.full(s, 3.0, device=dev) for k, s in (("means2D", (P, 3)), ("opacity", (P, 1)), ("means3D", (P, 3)),
                                                            ("scales", (P, 3)), ("rotations", (P, 4)))}
    _C.distortion_backward(over[4], over[5], over[6], torch.ones(1, H, W, device=dev), d, m, rs, binning_capacity=100,
                           accumulate_into=acc, **inputs)
    assert all(bool((t == 3.0).all()) for t in acc.values())
    g = _C.distortion_backward(over[4], over[5], over[6], torch.ones(1, H, W, device=dev), d, m, rs, binning_capacity=100, **inputs)
    assert all(t is None or not t.any() for t in g.values())
    # write mode and accumulate mode of a view that holds: the same gradients
    G = torch.ones(1, H, W, device=dev)
    w = _C.distortion_backward(exact[4], exact[5], exact[6], G, d0, m0, rs, **inputs)
    acc = {k: torch.zeros_like(t) for k, t in w.items() if t is not None}
    _C.distortion_backward(exact[4], exact[5], exact[6], G, d0, m0, rs, accumulate_into=acc, **inputs)
    assert w["means3D"].any() and w["cov3D"] is None
    for k, t in acc.items():
        assert torch.equal(t, w[k]), k
    # P = 0: zeros, no buffer read (none is given)
    dz = torch.ones(1, H, W, device=dev)
    mz = torch.ones(H, W, 4, device=dev)
    a = _lib.DistortionArgs(P=0, width=W, height=H, map_c1=1.0, out_distortion=dz.data_ptr(), out_moments=mz.data_ptr(), stream=stream)
    assert L.lr_render_distortion(a) == 0
    torch.cuda.synchronize()
    assert not dz.any() and not mz.any()
    # a wrong struct_bytes and a missing required pointer, with everything else in place
    a = _lib.DistortionArgs(geom_buffer=exact[4].data_ptr(), binning_buffer=exact[5].data_ptr(), image_buffer=exact[6].data_ptr(),
                            P=P, width=W, height=H, map_c1=1.0, out_distortion=dz.data_ptr(), out_moments=mz.data_ptr(), stream=stream)
    a.struct_bytes = ctypes.sizeof(_lib.DistortionArgs) - 8
    assert L.lr_render_distortion(a) == _lib.LR_ERR_INVALID_ARG
    a.struct_bytes = ctypes.sizeof(_lib.DistortionArgs)
    a.out_moments = None
    assert L.lr_render_distortion(a) == _lib.LR_ERR_INVALID_ARG and b"required" in L.lr_last_error()
    b = _lib.DistortionBackwardArgs()
    b.struct_bytes += 8
    assert L.lr_distortion_backward(b) == _lib.LR_ERR_INVALID_ARG
    with pytest.raises(RuntimeError, match="scales"):
        _C.distortion_backward(exact[4], exact[5], exact[6], G, d0, m0, rs, means3D=inputs["means3D"], raw=True,
                               opacities=cloud["opacities"].to(dev))          # raw mode without scaling / rotation
    torch.cuda.synchronize()


def test_render_and_install_pass_distortion_through(hip_device):
    from types import SimpleNamespace
    from luciddreamer_amd import cameras, dropin
    from luciddreamer_amd.gaussian_renderer import render, render_raw
    W, H = 128, 96
    pc = _raw_cloud(synthetic.make_cloud(5_000, "band", 4), 1, hip_device)
    cam = cameras.rotate360_path(W, H, n_views=12)[0].to(hip_device)
    b = render_raw(cam, pc, render_only=True, return_distortion=True)
    assert set(b) == {"render", "depth", "distortion"} and "distortion" not in render(cam, pc)
    lin = render_raw(cam, pc, return_distortion=True, distortion_map="linear")
    assert (b["distortion"] > 0).any() and not torch.equal(lin["distortion"], b["distortion"])
    all3 = render(cam, pc, return_alpha=True, return_median=True, return_distortion=True)
    assert all3["alpha"].shape == all3["distortion"].shape == (1, H, W) and all3["median_ids"].dtype == torch.int32

    def reference_render(*args, **kw):
        raise AssertionError("the reference's render cannot return the distortion")
    ns = SimpleNamespace(render=reference_render)
    opt = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    h = dropin.install(ns, None, None, losses=False, adam=False, stats=False)
    try:
        out = ns.render(cam, pc, opt, torch.zeros(3, device=hip_device), return_distortion=True)
        over = ns.render(cam, pc, opt, torch.zeros(3, device=hip_device), override_color=torch.ones_like(pc._xyz),
                         return_distortion=True, distortion_map="linear")
    finally:
        dropin.uninstall(h)
    assert torch.equal(out["distortion"], b["distortion"])
    assert over["distortion"].shape == (1, H, W) and (over["distortion"] > 0).any()
