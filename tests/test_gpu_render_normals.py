"""Rendered normal map on the GPU (return_normals -> lr_render_normals, lr_render_normals_backward).

The forward against the float64 reference (tests/render_normals_ref.py; its own properties and the measured float32 error the bar
comes from: tests/test_render_normals_cpu.py) under default and strict evaluation and both entry points; every leaf's gradient
against float64 autograd at GRAD_RTOL; the per-Gaussian normals and their gradient through the C ABI; the crafted cloud; how the
term composes with the colour and the distortion backward, fused accumulation and the armed optimizer step; the output order;
anti-aliasing; the edges of the C ABI; the consistency helper.  Every test fails without the feature: return_normals and the entry
points do not exist there."""
import ctypes

import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, config, synthetic
from tests import distort_ref as dr, helpers as hp, render_normals_ref as rn

pytestmark = pytest.mark.gpu

NAMES = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
REF_KEY = dict(means3D="means3D", means2D="means2D", opacities="opacity", shs="sh", scales="scales", rotations="rotations")
GEO = ["means3D", "means2D", "opacity", "scales", "rotations"]
RAW = (("xyz", "_xyz"), ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"))
FWD_BAR = 4.0                           # x render_normals_ref.FWD_ERR (its comment)


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


def _run(cloud, cam, degree, bg, dev, gc=None, gn=None, gd=None, normals=True, distortion=False, alpha=False, median=False,
         fused=False):
    """GaussianRasterizer on fresh leaves; loss <gc, color> + <gn, normals> + <gd, distortion> (terms left out when None)."""
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
    if normals:
        kw["return_normals"] = True
    if distortion:
        kw["return_distortion"] = True
    H, W = cam.image_height, cam.image_width
    config.set_fused_grad_accumulation(fused)
    try:
        out = GaussianRasterizer(_settings(cam, bg, degree, dev))(**leaves, **kw)
        # the documented order: colour, radii, depth, [alpha], [median_depth, median_ids], [normals], [distortion]
        assert len(out) == 3 + bool(alpha) + 2 * bool(median) + bool(normals) + bool(distortion)
        res = dict(color=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy(), depth=out[2].detach().cpu().numpy())
        k = 3
        if alpha:
            assert out[k].shape == (1, H, W)
            res["alpha"] = out[k].detach().cpu().numpy()
            k += 1
        if median:
            assert out[k].shape == (1, H, W) and out[k + 1].shape == (H, W) and out[k + 1].dtype == torch.int32
            res["median_depth"], res["median_ids"] = out[k].detach().cpu().numpy(), out[k + 1].cpu().numpy()
            k += 2
        t_n = t_d = None
        if normals:
            t_n = out[k]
            assert t_n.shape == (3, H, W) and t_n.dtype == torch.float32
            res["normals"] = t_n.detach().cpu().numpy()
            k += 1
        if distortion:
            t_d = out[k]
            assert t_d is out[-1] and t_d.shape == (1, H, W)          # distortion stays the last output
            res["distortion"] = t_d.detach().cpu().numpy()
        loss = None
        for t, g in ((out[0], gc), (t_n, gn), (t_d, gd)):
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


def _run_raw(cloud, cam, degree, bg, dev, gn=None):
    from luciddreamer_amd.gaussian_renderer import render_raw
    pc = _raw_cloud(cloud, degree, dev)
    out = render_raw(cam.to(dev), pc, bg_color=bg.to(dev), return_normals=True)
    res = dict(normals=out["normals"].detach().cpu().numpy())
    if gn is not None:
        (out["normals"] * gn.to(dev)).sum().backward()
        res["grads"] = {k: getattr(pc, a).grad.cpu().numpy() for k, a in RAW}
        res["grads"]["means2D"] = out["viewspace_points"].grad.cpu().numpy()
        res["grads"]["features_dc"] = pc._features_dc.grad.cpu().numpy()
        res["grads"]["features_rest"] = pc._features_rest.grad.cpu().numpy()
    return res


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _forward_c_abi(cloud, cam, dev, capacity):
    from luciddreamer_amd import _C
    tfx, tfy = hp.tan_fov(cam)
    camd = cam.to(dev)
    return _C.rasterize_gaussians(torch.zeros(3, device=dev), cloud["means3D"].to(dev), torch.Tensor([]),
                                  cloud["opacities"].to(dev), cloud["scales"].to(dev), cloud["rotations"].to(dev), 1.0,
                                  torch.Tensor([]), camd.world_view_transform, camd.full_proj_transform, tfx, tfy,
                                  cam.image_height, cam.image_width, cloud["shs"].to(dev), 3, camd.camera_center, False, False,
                                  binning_capacity=capacity)


# ---- 1. forward parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("name", rn.NAMES)
def test_forward_parity_with_the_float64_reference(hip_device, exact_mode, name, strict):
    """Every component of every non-fragile pixel within 4 x the float32 walk's own measured error; exact zeros where the
    reference has no layer; on "sparse" and "posed" the raw entry point too (log-scales pick the same axis: asserted on the CPU)."""
    cam, cloud, degree, bg = rn.case(name)
    r = rn.reference(name)
    ok = ~r["fragile"]
    assert r["fragile"].sum() <= rn.FRAGILE_CAP * r["fragile"].size
    bar = FWD_BAR * rn.FWD_ERR[name]
    config.set_strict_parity(strict)
    outs = {}
    try:
        outs["activated"] = _run(cloud, cam, degree, bg, hip_device)["normals"]
        if name in ("sparse", "posed"):
            outs["raw"] = _run_raw(cloud, cam, degree, bg, hip_device)["normals"]
    finally:
        config.set_strict_parity(False)
    for key, N in outs.items():
        err = float(np.abs(N.astype(np.float64) - r["N64"])[:, ok].max())
        print(name, "strict" if strict else "default", key, "err %.3e" % err, "bar %.3e" % bar)
    for key, N in outs.items():
        err = float(np.abs(N.astype(np.float64) - r["N64"])[:, ok].max())
        assert err <= bar, (key, err, bar)
        assert not N[:, ok & (r["layers64"] == 0)].any(), key
        assert N[:, ok & (r["layers64"] > 0)].any(), key


# ---- 2. gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("name", ["sparse", "dense", "wide", "posed"])
def test_gradients_against_float64_autograd(hip_device, exact_mode, name, strict):
    """Every leaf at GRAD_RTOL for a seeded upstream that is zero on the fragile pixels (on both sides); colour and SH gradients
    are exact zeros when only N carries a gradient."""
    cam, cloud, degree, bg = rn.case(name)
    r = rn.reference(name)
    config.set_strict_parity(strict)
    try:
        act = _run(cloud, cam, degree, bg, hip_device, gn=r["G"])
    finally:
        config.set_strict_parity(False)
    got = {REF_KEY[k]: v for k, v in act["grads"].items()}
    for k in GEO:
        ref = r["leaf"][k]
        print(name, k, "err %.2e of max |g| = %.3e" % (np.abs(got[k].reshape(ref.shape) - ref).max() / np.abs(ref).max(),
                                                       np.abs(ref).max()))
    hp.compare_grads(got, r["leaf"], names=GEO)
    assert not act["grads"]["shs"].any()


def test_raw_mode_gradients(hip_device, exact_mode):
    """The stored parameters' gradients on "posed": the quaternion-normalisation Jacobian of the normal's chain included."""
    name = "posed"
    cam, cloud, degree, bg = rn.case(name)
    r = rn.reference(name)
    raw = _run_raw(cloud, cam, degree, bg, hip_device, gn=r["G"])
    want = rn.raw_grads(cloud, r["leaf"])
    for k in want:
        print(name, "raw", k, "err %.2e" % (np.abs(raw["grads"][k].reshape(want[k].shape) - want[k]).max() / np.abs(want[k]).max()))
    hp.compare_grads(raw["grads"], want, names=list(want))
    assert not raw["grads"]["features_dc"].any() and not raw["grads"]["features_rest"].any()
    # the normalisation Jacobian is at work: the gradient has no component along the stored quaternion
    q = cloud["rotations"].double().numpy()
    along = np.abs((raw["grads"]["rotation"].astype(np.float64) * q).sum(axis=1)).max()
    assert along <= hp.GRAD_RTOL * np.abs(want["rotation"]).max()


@pytest.mark.parametrize("name", ["sparse", "posed"])
def test_gauss_normals_and_their_gradient_through_the_c_abi(hip_device, name):
    from luciddreamer_amd import _C
    cam, cloud, degree, bg = rn.case(name)
    r = rn.reference(name)
    dev = hip_device
    rs = _settings(cam, torch.zeros(3), 3, dev)
    inputs = dict(means3D=cloud["means3D"].to(dev), scales=cloud["scales"].to(dev), rotations=cloud["rotations"].to(dev))
    f = _forward_c_abi(cloud, cam, dev, 0)
    N, gn = _C.render_normals(f[4], f[5], f[6], f[3], rs, **inputs)
    gn_h, vis = gn.cpu().numpy(), r["visible"]
    assert np.array_equal(f[3].cpu().numpy() > 0, vis)
    assert not gn_h[~vis].any()                                               # rows with radii <= 0 are zeros
    assert np.array_equal(gn_h[vis, 3], r["sign"][vis] * (r["k"][vis] + 1))   # axis and sign: the reference's, exactly
    err = np.abs(gn_h[vis, :3] - r["gn64"][vis]).max()
    print(name, "gauss_normals err %.3e" % err)
    assert err <= 2e-6                          # a unit vector through ~20 float32 operations on values <= 2 (the CPU statement holds the same)
    out = _C.render_normals_backward(f[4], f[5], f[6], r["G"].to(dev), N, gn, f[3], rs, **inputs)
    dn = out["gauss_normal"].cpu().numpy()
    ref = r["mid"]["n"]
    print(name, "dL_dgauss_normal err %.2e of max %.3e" % (np.abs(dn - ref).max() / np.abs(ref).max(), np.abs(ref).max()))
    hp.compare_grads(dict(n=dn), dict(n=ref), names=["n"])
    assert not dn[~vis].any()


# ---- 3. the crafted cloud -----------------------------------------------------------------------------------------------------
def test_crafted_cloud_on_the_device(hip_device):
    """Axis, flip and the isotropic tie, and the discs against the depth normals of their plane."""
    from luciddreamer_amd import _C, normals
    cam, cloud, degree, bg, expect = rn.crafted()
    dev = hip_device
    rs = _settings(cam, bg, degree, dev)
    inputs = dict(means3D=cloud["means3D"].to(dev), scales=cloud["scales"].to(dev), rotations=cloud["rotations"].to(dev))
    f = _forward_c_abi(cloud, cam, dev, 0)
    N, gn = _C.render_normals(f[4], f[5], f[6], f[3], rs, **inputs)
    gn = gn.cpu().numpy()
    _, N64, layers, inter = rn.render64(cloud, cam, degree, bg)
    # sign (k + 1): the isotropic one takes axis 0; the discs' signs are known by hand, the tilted ones' from the reference
    assert np.abs(gn[:, 3]).tolist() == [1.0, 2.0, 3.0, 1.0, 3.0, 3.0] and gn[4:, 3].tolist() == [-3.0, 3.0]
    assert np.sign(gn[:, 3]).tolist() == inter["sign"].tolist()
    for i, (_, want) in expect.items():
        assert np.abs(gn[i, :3] - want).max() <= 1e-6, i
    assert np.array_equal(gn[4, :3], gn[5, :3])                               # towards and away: the same normal after the flip
    out = _run(cloud, cam, degree, bg, dev, alpha=True)
    Nh, alpha = out["normals"], out["alpha"][0]
    assert np.array_equal(Nh, N.cpu().numpy())
    assert np.abs(Nh - N64.detach().numpy()).max() <= 1e-6                    # one layer per pixel: alpha's own float32 error
    assert not Nh[:, layers.numpy() == 0].any()
    disc = (layers.numpy() > 0) & (np.arange(rn.CRAFT_H)[:, None] > rn.CRAFT_H // 2) & (np.arange(rn.CRAFT_W)[None, :] > 22)
    # N = (0, 0, -w) with w the one layer's alpha; the alpha OUTPUT is 1 - (1 - w): two more roundings of values <= 1
    assert not Nh[0][disc].any() and not Nh[1][disc].any() and np.abs(Nh[2][disc] + alpha[disc]).max() <= 2.0 ** -23
    # the rendered normal / alpha against depth_normals of the rendered depth, where that is valid (inside a disc: the plane z = 4)
    dn = normals.depth_normals(torch.from_numpy(out["depth"]).to(dev), cam.to(dev)).cpu().numpy()
    both = disc & (dn != 0).any(axis=0)
    assert both.sum() > 20
    # the rendered depth is 4 w / (w + 1e-6) where w > 0.5: within 8e-6 + float32 rounding of the plane, so a central difference
    # over two pixels (0.11 view units at z = 4) tilts the depth normal by at most 1.7e-5 / 0.11 = 1.5e-4 (x 1.1 for the ray slope)
    assert np.abs(Nh[:, both] / alpha[both] - dn[:, both]).max() <= 3e-4


# ---- 4. composition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "posed"])
def test_composition_with_the_colour_and_distortion_backward(hip_device, exact_mode, name):
    cam, cloud, degree, bg = rn.case(name)
    H, W = cam.image_height, cam.image_width
    r = rn.reference(name)
    d = dr.reference(name, "ndc")
    gn = r["G"].clone()                 # (both upstreams: zero on the pixels either reference calls fragile)
    gn[:, torch.from_numpy(np.array(d["fragile"]))] = 0.0
    gd = d["G"] * 1000.0                # the "ndc" distortion is small: an upstream that brings its gradient to the others' size
    gd[:, torch.from_numpy(np.array(r["fragile"]))] = 0.0
    gc = synthetic.upstream_grad(H, W)
    # float64: colour + normals in one autograd pass; the distortion's gradient is linear in its upstream
    cn64, _, _, _, _ = rn.grads64(cloud, cam, degree, bg, gn.numpy(), gc=gc)
    d64, _, _, _ = dr.grads64(cloud, cam, degree, bg, dr.coefficients("ndc"), gd.numpy())
    cdn64 = {k: cn64[k] + d64[k] for k in cn64}
    colour = _run(cloud, cam, degree, bg, hip_device, gc=gc, normals=False)
    alone = _run(cloud, cam, degree, bg, hip_device, gn=gn)
    two = _run(cloud, cam, degree, bg, hip_device, gc=gc, gn=gn)
    three = _run(cloud, cam, degree, bg, hip_device, gc=gc, gn=gn, gd=gd, distortion=True)
    for label, got, want in (("colour + normals", two, cn64), ("colour + distortion + normals", three, cdn64)):
        g = {REF_KEY[k]: v for k, v in got["grads"].items()}
        for k in GEO + ["sh"]:
            print(name, label, k, "err %.2e of max %.3e" % (np.abs(g[k].reshape(want[k].shape) - want[k]).max() / np.abs(want[k]).max(),
                                                            np.abs(want[k]).max()))
        hp.compare_grads(g, want, names=GEO + ["sh"])
    for k in GEO:                                                     # the term is not lost against the colour's
        kk = [n for n in NAMES if REF_KEY[n] == k][0]
        assert np.abs(alone["grads"][kk]).max() > 0.01 * np.abs(colour["grads"][kk]).max(), k
    # fused gradient accumulation on: the same bits; two runs: the same bits, forward and backward
    for base, kw in ((two, dict()), (three, dict(gd=gd, distortion=True))):
        fused = _run(cloud, cam, degree, bg, hip_device, gc=gc, gn=gn, fused=True, **kw)
        again = _run(cloud, cam, degree, bg, hip_device, gc=gc, gn=gn, **kw)
        assert np.array_equal(_bits(again["normals"]), _bits(base["normals"]))
        for k in NAMES:
            differ = _bits(fused["grads"][k]) != _bits(base["grads"][k])
            print(name, k, "fused against unfused:", int(differ.sum()), "words differ, by",
                  float(np.abs(fused["grads"][k] - base["grads"][k]).max()), "at most")
            assert np.array_equal(_bits(again["grads"][k]), _bits(base["grads"][k])), k
            assert np.array_equal(_bits(fused["grads"][k]), _bits(base["grads"][k])), k
    # an unused normals output (with unused alpha, median and distortion outputs next to it): the colour gradients' bits
    unused = _run(cloud, cam, degree, bg, hip_device, gc=gc, alpha=True, median=True, distortion=True)
    for k in ("color", "depth", "radii"):
        assert np.array_equal(unused[k], colour[k]), k
    for k in NAMES:
        assert np.array_equal(_bits(unused["grads"][k]), _bits(colour["grads"][k])), k
    # all requested: each output is what it is when requested alone
    assert np.array_equal(_bits(unused["normals"]), _bits(two["normals"]))
    assert np.array_equal(_bits(unused["distortion"]), _bits(three["distortion"]))


def test_output_order_with_every_optional_output(hip_device):
    """colour, radii, depth, alpha, median_depth, median_ids, normals, distortion (asserted inside _run), through both entry points."""
    from luciddreamer_amd.gaussian_renderer import render_raw
    from luciddreamer_amd.rasterizer import rasterize_gaussians_raw
    cam, cloud, degree, bg = rn.case("thin")
    H, W = cam.image_height, cam.image_width
    out = _run(cloud, cam, degree, bg, hip_device, alpha=True, median=True, distortion=True)
    only = _run(cloud, cam, degree, bg, hip_device)
    assert np.array_equal(_bits(out["normals"]), _bits(only["normals"])) and out["normals"].any()
    pc = _raw_cloud(cloud, degree, hip_device)
    rs = _settings(cam, bg, degree, hip_device)
    raw = rasterize_gaussians_raw(pc._xyz, torch.zeros_like(pc._xyz), pc._features_dc, pc._features_rest, pc._opacity, pc._scaling,
                                  pc._rotation, rs, return_alpha=True, return_median=True, return_distortion=True, return_normals=True)
    assert [tuple(t.shape) for t in raw[3:]] == [(1, H, W), (1, H, W), (H, W), (3, H, W), (1, H, W)]
    pkg = render_raw(cam.to(hip_device), pc, bg_color=bg.to(hip_device), return_alpha=True, return_median=True, return_distortion=True,
                     return_normals=True)
    assert torch.equal(pkg["normals"], raw[6]) and torch.equal(pkg["distortion"], raw[7]) and torch.equal(pkg["alpha"], raw[3])


# ---- 5. wrappers --------------------------------------------------------------------------------------------------------------
def test_render_and_install_pass_normals_through(hip_device):
    from types import SimpleNamespace
    from luciddreamer_amd import cameras, dropin
    from luciddreamer_amd.gaussian_renderer import render, render_raw
    W, H = 128, 96
    pc = _raw_cloud(synthetic.make_cloud(5_000, "band", 4), 1, hip_device)
    cam = cameras.rotate360_path(W, H, n_views=12)[0].to(hip_device)
    b = render_raw(cam, pc, render_only=True, return_normals=True)
    assert set(b) == {"render", "depth", "normals"} and "normals" not in render(cam, pc)
    assert b["normals"].shape == (3, H, W) and b["normals"].any()
    a = render(cam, pc, return_alpha=True, return_normals=True)
    assert float((a["normals"].detach().norm(dim=0) - a["alpha"][0].detach()).max()) <= 1e-5                # |N| <= alpha
    pc.get_covariance = lambda scaling_modifier=1.0: torch.zeros(pc._xyz.shape[0], 6, device=hip_device)     # GaussianModel's getter
    with pytest.raises(ValueError, match="cov3D_precomp"):
        render(cam, pc, SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=False), return_normals=True)

    def reference_render(*args, **kw):
        raise AssertionError("the reference's render cannot return the normals")
    ns = SimpleNamespace(render=reference_render)
    opt = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    h = dropin.install(ns, None, None, losses=False, adam=False, stats=False)
    try:
        out = ns.render(cam, pc, opt, torch.zeros(3, device=hip_device), return_normals=True)
        over = ns.render(cam, pc, opt, torch.zeros(3, device=hip_device), override_color=torch.ones_like(pc._xyz),
                         return_normals=True)
    finally:
        dropin.uninstall(h)
    assert torch.equal(out["normals"], b["normals"])
    assert over["normals"].shape == (3, H, W) and over["normals"].any()


def test_armed_fused_step_takes_the_normals_gradient(hip_device):
    """The armed FusedAdam (raw node's no-zero-fill backward + masked step) with a colour + normals loss: the same parameter
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
        gn = torch.randn(3, H, W, generator=gen).to(hip_device)
        pa = render_raw(cam, a, bg_color=bg, return_normals=True)
        ((pa["render"] * g).sum() + (pa["normals"] * gn).sum()).backward()
        opt_a.step()
        opt_a.zero_grad(set_to_none=True)
        assert opt_b.arm_fused_backward()
        pb = render_raw(cam, b, bg_color=bg, return_normals=True)
        ((pb["render"] * g).sum() + (pb["normals"] * gn).sum()).backward()
        assert all(getattr(b, n).grad is None for n in params)
        opt_b.step()
        opt_b.zero_grad(set_to_none=True)
        moved |= bool(pa["normals"].any())
        assert torch.equal(pa["normals"], pb["normals"]), it
        for n in params:
            assert torch.equal(getattr(a, n), getattr(b, n)), (it, n)
    assert moved


# ---- 6. anti-aliasing ---------------------------------------------------------------------------------------------------------
def test_gradients_with_antialiasing_on(hip_device, exact_mode):
    """The blend sees opacity x coef (tests/aa_ref.py): the reference is fed the compensated opacity, whose own derivative reaches
    the scales."""
    cam, cloud, degree, bg = rn.case("sparse")
    r = rn.aa_reference("sparse")
    plain = rn.reference("sparse")
    assert np.abs(r["leaf"]["scales"] - plain["leaf"]["scales"]).max() > 100 * hp.GRAD_RTOL * np.abs(plain["leaf"]["scales"]).max()
    config.set_antialiasing(True)
    try:
        got = _run(cloud, cam, degree, bg, hip_device, gn=r["G"])
    finally:
        config.set_antialiasing(False)
    ok = ~r["fragile"]
    assert np.abs(got["normals"].astype(np.float64) - r["N64"])[:, ok].max() <= FWD_BAR * rn.FWD_ERR["sparse"]
    g = {REF_KEY[k]: v for k, v in got["grads"].items()}
    hp.compare_grads(g, r["leaf"], names=GEO)


# ---- 7. edges of the C ABI ----------------------------------------------------------------------------------------------------
def test_c_abi_edges(hip_device):
    from luciddreamer_amd import _C, cameras
    cam, cloud, _, _ = rn.case("sparse")
    H, W, P = cam.image_height, cam.image_width, cloud["means3D"].shape[0]
    dev = hip_device
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rs = _settings(cam, torch.zeros(3), 3, dev)
    inputs = dict(means3D=cloud["means3D"].to(dev), scales=cloud["scales"].to(dev), rotations=cloud["rotations"].to(dev))
    exact = _forward_c_abi(cloud, cam, dev, 0)
    n0, g0 = _C.render_normals(exact[4], exact[5], exact[6], exact[3], rs, **inputs)
    assert n0.any() and g0.shape == (P, 4)
    # a capacity that holds the view: the exact forward's outputs
    cap = 4 * int(exact[0]) + 1024
    roomy = _forward_c_abi(cloud, cam, dev, cap)
    n1, g1 = _C.render_normals(roomy[4], roomy[5], roomy[6], roomy[3], rs, binning_capacity=cap, **inputs)
    assert torch.equal(n0, n1) and torch.equal(g0, g1)
    # an async forward whose binning capacity is too small: zeros, rc 0, the overflow is lr_check's to report; the backward adds nothing
    over = _forward_c_abi(cloud, cam, dev, 100)
    n, g = _C.render_normals(over[4], over[5], over[6], over[3], rs, binning_capacity=100, **inputs)
    assert not n.any()
    with pytest.raises(RuntimeError, match="capacity"):
        _C.check(over[4])
    G = torch.ones(3, H, W, device=dev)
    acc = {k: torch.full(s, 3.0, device=dev) for k, s in (("means2D", (P, 3)), ("opacity", (P, 1)), ("means3D", (P, 3)),
                                                            ("scales", (P, 3)), ("rotations", (P, 4)))}
    o = _C.render_normals_backward(over[4], over[5], over[6], G, n, g, over[3], rs, binning_capacity=100, accumulate_into=acc, **inputs)
    assert all(bool((t == 3.0).all()) for t in acc.values()) and not o["gauss_normal"].any()
    o = _C.render_normals_backward(over[4], over[5], over[6], G, n, g, over[3], rs, binning_capacity=100, **inputs)
    assert all(not t.any() for t in o.values())
    # write mode and accumulate mode of a view that holds: the same gradients
    w = _C.render_normals_backward(exact[4], exact[5], exact[6], G, n0, g0, exact[3], rs, **inputs)
    acc = {k: torch.zeros_like(t) for k, t in w.items() if k != "gauss_normal"}
    w2 = _C.render_normals_backward(exact[4], exact[5], exact[6], G, n0, g0, exact[3], rs, accumulate_into=acc, **inputs)
    assert w["means3D"].any() and w["rotations"].any() and torch.equal(w["gauss_normal"], w2["gauss_normal"])
    for k, t in acc.items():
        assert torch.equal(t, w[k]), k
    # P = 0: zeros, no buffer read (none is given)
    nz = torch.ones(3, H, W, device=dev)
    a = _lib.NormalsRenderArgs(view=_lib.View(P=0, width=W, height=H), out_normals=nz.data_ptr(), stream=stream)
    assert L.lr_render_normals(a) == 0
    torch.cuda.synchronize()
    assert not nz.any()
    # a 1 x 1 and a 17 x 16 image: a tile with one pixel, and a second tile column one pixel wide
    for (w_, h_) in ((1, 1), (17, 16)):
        c = cameras.identity_camera(w_, h_)
        f = _forward_c_abi(cloud, c, dev, 0)
        rs_ = _settings(c, torch.zeros(3), 3, dev)
        nn_, gg_ = _C.render_normals(f[4], f[5], f[6], f[3], rs_, **inputs)
        st = hp.run_oracle(cloud, c, 3, torch.zeros(3))
        gn32 = rn.gauss_normals32(cloud["means3D"].numpy(), cloud["scales"].numpy(), cloud["rotations"].numpy(),
                                  c.world_view_transform.numpy(), st["radii"])
        N32, layers32, fragile = rn.walk32(st["res"].stage(), w_, h_, gn32)
        assert nn_.shape == (3, h_, w_) and (layers32.max() > 0 or (w_, h_) == (1, 1))
        err = np.abs(nn_.cpu().numpy() - N32)[:, ~fragile].max() if (~fragile).any() else 0.0
        print("%d x %d: err against the float32 walk %.3e" % (w_, h_, err))
        assert err <= FWD_BAR * max(rn.FWD_ERR.values())
        o = _C.render_normals_backward(f[4], f[5], f[6], torch.ones(3, h_, w_, device=dev), nn_, gg_, f[3], rs_, **inputs)
        assert all(bool(torch.isfinite(t).all()) for t in o.values()) and (o["rotations"].any() or layers32.max() == 0)
    # a wrong struct_bytes and a missing required pointer, with everything else in place
    a = _lib.NormalsRenderArgs(view=_lib.View(P=P, width=W, height=H), geom_buffer=exact[4].data_ptr(),
                               binning_buffer=exact[5].data_ptr(), image_buffer=exact[6].data_ptr(), out_normals=nz.data_ptr(),
                               stream=stream)
    assert L.lr_render_normals(a) == _lib.LR_ERR_INVALID_ARG and b"required" in L.lr_last_error()
    a.struct_bytes = ctypes.sizeof(_lib.NormalsRenderArgs) - 8
    assert L.lr_render_normals(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    with pytest.raises(ValueError, match="cov3D_precomp"):
        _C.render_normals(exact[4], exact[5], exact[6], exact[3], rs, means3D=inputs["means3D"], scales=None, rotations=None,
                          cov3D_precomp=torch.zeros(P, 6, device=dev))
    torch.cuda.synchronize()


# ---- 8. the consistency helper ------------------------------------------------------------------------------------------------
def test_rendered_normal_consistency_against_its_float64_restatement(hip_device):
    """weight * sum_valid (1 - N . n) / (H W) on "sparse": the value and both gradients against the float64 torch statement
    (tests/normal_ref.torch_normals for n: lifted points, autograd), evaluated on the device's own N and depth."""
    from luciddreamer_amd import normals
    from tests import normal_ref as nr
    cam, cloud, degree, bg = rn.case("sparse")
    H, W = cam.image_height, cam.image_width
    out = _run(cloud, cam, degree, bg, hip_device)
    tx, ty = hp.tan_fov(cam)
    weight = 0.7
    N = torch.from_numpy(out["normals"]).to(hip_device).requires_grad_(True)
    depth = torch.from_numpy(out["depth"]).to(hip_device).requires_grad_(True)
    loss = normals.rendered_normal_consistency(N, depth, cam.to(hip_device), weight=weight)
    loss.backward()
    N64 = torch.from_numpy(out["normals"]).double().requires_grad_(True)
    d64 = torch.from_numpy(out["depth"][0]).double().requires_grad_(True)
    n64, valid = nr.torch_normals(d64, tx, ty)
    want = weight * torch.where(valid, 1.0 - (N64 * n64).sum(0), torch.zeros(H, W, dtype=torch.float64)).sum() / (H * W)
    want.backward()
    n_dev = normals.depth_normals(depth.detach(), cam.to(hip_device)).cpu().numpy()
    assert np.array_equal((n_dev != 0).any(axis=0), valid.numpy()) and valid.sum() > 0.3 * H * W
    # The bars.  The helper adds three float32 torch ops to depth_normals, so its error is depth_normals' own carried through sums
    # of H W terms of size <= |N| <= 1, plus the float32 rounding of those sums.  depth_normals' own error on THIS depth map is
    # calibrated as tests/test_gpu_normals.py calibrates it: by the float32 restatement of the header's closed form (e32), with
    # that suite's margin (rowbar.E32_MARGIN) and floor.
    from tests import rowbar
    n32, _ = nr.closed_normals(out["depth"][0], tx, ty, np.float32)
    e_n = max(rowbar.E32_MARGIN * float(np.abs(n32 - n64.detach().numpy()).max()), 16 * 2.0 ** -24)
    loss_v, want_v = float(loss.detach()), float(want.detach())
    print("e_n %.3e" % e_n, "loss %.6f" % loss_v, "want %.6f" % want_v)
    assert abs(loss_v - want_v) <= weight * (3 * e_n + 2.0 ** -20)
    gN, gN64 = N.grad.cpu().numpy(), N64.grad.numpy()
    assert np.abs(gN - gN64).max() <= (weight / (H * W)) * (e_n + 2.0 ** -22)     # dL/dN = -weight n / (H W) on the valid pixels
    assert not gN[:, ~valid.numpy()].any()
    # dL/ddepth: depth_normals' backward of the upstream -weight N / (H W), held to that suite's gradient bar: 4 x the float32
    # restatements' own distance from float64 (both gather orders), or 1e-6 of the largest entry
    Gn = (-(weight / (H * W)) * out["normals"].astype(np.float64))
    g32 = [nr.closed_form_vjp(out["depth"][0], Gn.astype(np.float32), tx, ty, np.float32, order=o) for o in ("WENS", "SNEW")]
    gd, gd64 = depth.grad.cpu().numpy()[0].astype(np.float64), d64.grad.numpy()
    e32 = max(float(np.abs(np.asarray(g, np.float64) - gd64).max()) for g in g32)
    gmax = float(np.abs(gd64).max())
    print("dL/ddepth err %.3e = %.2e of max %.3e; float32 restatements within %.3e" % (np.abs(gd - gd64).max(), np.abs(gd - gd64).max() / gmax, gmax, e32))
    assert gmax > 0 and np.abs(gd - gd64).max() <= max(rowbar.E32_MARGIN * e32, 1e-6 * gmax)
