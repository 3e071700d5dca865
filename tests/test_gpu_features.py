"""N-channel feature map on the GPU (features= -> lr_render_features, lr_render_features_backward).

The forward against the float64 reference (tests/feature_ref.py: the workaround of ceil(C/3) colour renders in float64; its own
properties and the measured float32 error the bar comes from: tests/test_features_cpu.py) under default and strict evaluation,
both entry points and every channel count; the colour cross-check; every leaf's and the table's gradient against float64 autograd
at GRAD_RTOL; chunk independence bit for bit; how the term composes with the colour, normals and distortion backward, fused
accumulation and the armed optimizer step; the output order; anti-aliasing; the edges of the C ABI.  Every test fails without the
feature: the argument and the entry points do not exist there."""
import ctypes

import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, config, synthetic
from tests import distort_ref as dr, feature_ref as fr, helpers as hp, render_normals_ref as rn

pytestmark = pytest.mark.gpu

NAMES = ("means3D", "means2D", "opacities", "shs", "scales", "rotations", "features")
REF_KEY = dict(means3D="means3D", means2D="means2D", opacities="opacity", shs="sh", scales="scales", rotations="rotations",
               features="features")
GEO = ["means3D", "means2D", "opacity", "scales", "rotations"]
RAW = (("xyz", "_xyz"), ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"))
FWD_BAR = 4.0                           # x feature_ref.FWD_ERR (its comment)
K = fr.K


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


def _run(cloud, cam, degree, bg, dev, feats=None, gc=None, gf=None, gn=None, gd=None, normals=False, distortion=False, alpha=False,
         median=False, fused=False, colors=None, cov3D=None):
    """GaussianRasterizer on fresh leaves; loss <gc, color> + <gf, feature_map> + <gn, normals> + <gd, distortion> (terms left out
    when None).  colors: colors_precomp in place of the SHs; cov3D: cov3D_precomp in place of scales + rotations."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizer
    src = dict(cloud, features=feats, colors_precomp=colors, cov3D_precomp=cov3D)
    keys = ["means3D", "opacities"] + (["colors_precomp"] if colors is not None else ["shs"]) + \
           (["cov3D_precomp"] if cov3D is not None else ["scales", "rotations"]) + (["features"] if feats is not None else [])
    leaves = {k: src[k].detach().to(dev).requires_grad_(True) for k in keys}
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
        # the documented order: colour, radii, depth, [alpha], [median_depth, median_ids], [normals], [feature_map], [distortion]
        assert len(out) == 3 + bool(alpha) + 2 * bool(median) + bool(normals) + (feats is not None) + bool(distortion)
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
        t_n = t_f = t_d = None
        if normals:
            t_n = out[k]
            assert t_n.shape == (3, H, W)
            res["normals"] = t_n.detach().cpu().numpy()
            k += 1
        if feats is not None:
            t_f = out[k]
            assert t_f.shape == (feats.shape[1], H, W) and t_f.dtype == torch.float32
            res["features"] = t_f.detach().cpu().numpy()
            k += 1
        if distortion:
            t_d = out[k]
            assert t_d is out[-1] and t_d.shape == (1, H, W)          # distortion stays the last output
            res["distortion"] = t_d.detach().cpu().numpy()
        loss = None
        for t, g in ((out[0], gc), (t_f, gf), (t_n, gn), (t_d, gd)):
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


def _run_raw(cloud, cam, degree, bg, dev, feats, gf=None):
    from luciddreamer_amd.gaussian_renderer import render_raw
    pc = _raw_cloud(cloud, degree, dev)
    table = feats.detach().to(dev).requires_grad_(True)
    out = render_raw(cam.to(dev), pc, bg_color=bg.to(dev), features=table)
    res = dict(features=out["features"].detach().cpu().numpy())
    if gf is not None:
        (out["features"] * gf.to(dev)).sum().backward()
        res["grads"] = {k: getattr(pc, a).grad.cpu().numpy() for k, a in RAW}
        res["grads"]["means2D"] = out["viewspace_points"].grad.cpu().numpy()
        res["grads"]["features_dc"] = pc._features_dc.grad.cpu().numpy()
        res["grads"]["features_rest"] = pc._features_rest.grad.cpu().numpy()
        res["grads"]["features"] = table.grad.cpu().numpy()
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
@pytest.mark.parametrize("name", fr.NAMES)
def test_forward_parity_with_the_float64_reference(hip_device, exact_mode, name, strict):
    """Every plane of every non-fragile pixel within 4 x the float32 walk's own measured error; exact zeros where the reference
    has no layer; 2K + 1 channels everywhere, every channel count on "sparse", the raw entry point on "sparse" and "posed"."""
    cam, cloud, degree, bg = fr.case(name)
    r = fr.reference(name)
    ok = ~r["fragile"]
    assert r["fragile"].sum() <= fr.FRAGILE_CAP * r["fragile"].size
    bar = FWD_BAR * fr.FWD_ERR[name]
    config.set_strict_parity(strict)
    outs = {}
    try:
        for C in (fr.CHANNELS if name == "sparse" else (fr.C_MAX,)):
            outs["activated", C] = _run(cloud, cam, degree, bg, hip_device, feats=r["feats"][:, :C].contiguous())["features"]
        if name in ("sparse", "posed"):
            outs["raw", fr.C_MAX] = _run_raw(cloud, cam, degree, bg, hip_device, r["feats"])["features"]
    finally:
        config.set_strict_parity(False)
    for (key, C), F in outs.items():
        err = float(np.abs(F.astype(np.float64) - r["F64"][:C])[:, ok].max())
        print(name, "strict" if strict else "default", key, "C = %d" % C, "err %.3e" % err, "bar %.3e" % bar)
    for (key, C), F in outs.items():
        assert F.shape[0] == C
        err = float(np.abs(F.astype(np.float64) - r["F64"][:C])[:, ok].max())
        assert err <= bar, (key, C, err, bar)
        assert not F[:, ok & (r["layers32"] == 0)].any(), (key, C)
        assert F[:, ok & (r["layers32"] > 0)].any(), (key, C)


# ---- 2. the colour cross-check ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "posed"])
def test_three_channels_are_the_colour_of_the_workaround(hip_device, exact_mode, name):
    """C = 3 against the colour output of a render with colors_precomp = features and background 0, both from the device: the
    definition is the workaround's."""
    cam, cloud, degree, _ = fr.case(name)
    f3 = fr.features_of(name, 3)
    out = _run(cloud, cam, degree, torch.zeros(3), hip_device, feats=f3, colors=f3)
    err = float(np.abs(out["features"] - out["color"]).max())
    print(name, "feature map against the colour output: %.3e" % err)
    assert err <= hp.COLOR_ATOL and out["features"].any()


# ---- 3. gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("name", ["sparse", "dense", "wide", "posed"])
def test_gradients_against_float64_autograd(hip_device, exact_mode, name, strict):
    """Every leaf and the table at GRAD_RTOL for a seeded upstream that is zero on the fragile pixels (on both sides); SH
    gradients are exact zeros when only F carries a gradient; rows of the table with radii <= 0 get exact zeros."""
    cam, cloud, degree, bg = fr.case(name)
    r = fr.reference(name)
    config.set_strict_parity(strict)
    try:
        act = _run(cloud, cam, degree, bg, hip_device, feats=r["feats"], gf=r["G"])
    finally:
        config.set_strict_parity(False)
    got = {REF_KEY[k]: v for k, v in act["grads"].items()}
    for k in GEO + ["features"]:
        ref = r["leaf"][k]
        print(name, k, "err %.2e of max |g| = %.3e" % (np.abs(got[k].reshape(ref.shape) - ref).max() / np.abs(ref).max(),
                                                       np.abs(ref).max()))
    hp.compare_grads(got, r["leaf"], names=GEO + ["features"])
    assert not act["grads"]["shs"].any()
    assert np.array_equal(act["radii"] > 0, r["visible"]) and (~r["visible"]).any()
    assert not act["grads"]["features"][~r["visible"]].any()


def test_raw_mode_gradients(hip_device, exact_mode):
    """The stored parameters' gradients on "posed" through distort_ref.raw_grads; the table has no activation."""
    name = "posed"
    cam, cloud, degree, bg = fr.case(name)
    r = fr.reference(name)
    raw = _run_raw(cloud, cam, degree, bg, hip_device, r["feats"], gf=r["G"])
    want = dict(fr.raw_grads(cloud, r["leaf"]), features=r["leaf"]["features"])
    for k in want:
        print(name, "raw", k, "err %.2e" % (np.abs(raw["grads"][k].reshape(want[k].shape) - want[k]).max() / np.abs(want[k]).max()))
    hp.compare_grads(raw["grads"], want, names=list(want))
    assert not raw["grads"]["features_dc"].any() and not raw["grads"]["features_rest"].any()


def test_cov3d_precomp_takes_the_gradient(hip_device, exact_mode):
    """Nothing here needs scales or rotations: with cov3D_precomp the gradient reaches cov3D."""
    name = "sparse"
    cam, cloud, degree, bg = fr.case(name)
    r, c = fr.reference(name), fr.cov_reference(name)
    got = _run(cloud, cam, degree, bg, hip_device, feats=r["feats"], gf=r["G"], cov3D=c["cov3D"])
    ok = ~r["fragile"]
    assert float(np.abs(got["features"].astype(np.float64) - r["F64"])[:, ok].max()) <= FWD_BAR * fr.FWD_ERR[name]
    g = dict(means3D=got["grads"]["means3D"], means2D=got["grads"]["means2D"], opacity=got["grads"]["opacities"],
             cov3D=got["grads"]["cov3D_precomp"], features=got["grads"]["features"])
    for k in g:
        print(name, "cov3D_precomp", k, "err %.2e" % (np.abs(g[k].reshape(c["leaf"][k].shape) - c["leaf"][k]).max() / np.abs(c["leaf"][k]).max()))
    assert np.abs(c["leaf"]["cov3D"]).max() > 0
    hp.compare_grads(g, c["leaf"], names=list(g))


# ---- 4. chunk independence, bit for bit ---------------------------------------------------------------------------------------
def test_chunk_independence_bit_for_bit(hip_device, exact_mode):
    """The planes of features[:, a:b] rendered alone are the planes a:b of the full render, and the same for those columns of
    dL_dfeatures: a slice inside a chunk, one across a chunk boundary, and the tail.  A channel permutation permutes both."""
    name = "sparse"
    cam, cloud, degree, bg = fr.case(name)
    r = fr.reference(name)
    full = _run(cloud, cam, degree, bg, hip_device, feats=r["feats"], gf=r["G"])
    assert full["grads"]["features"].any()
    for a, b in ((3, 8), (K - 3, K + 5), (2 * K - 1, 2 * K + 1), (2 * K, 2 * K + 1)):
        part = _run(cloud, cam, degree, bg, hip_device, feats=r["feats"][:, a:b].contiguous(), gf=r["G"][a:b].contiguous())
        assert np.array_equal(_bits(part["features"]), _bits(full["features"][a:b])), (a, b)
        assert np.array_equal(_bits(part["grads"]["features"]), _bits(full["grads"]["features"][:, a:b])), (a, b)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(fr.C_MAX))
    p = _run(cloud, cam, degree, bg, hip_device, feats=r["feats"][:, perm].contiguous(), gf=r["G"][perm].contiguous())
    assert np.array_equal(_bits(p["features"]), _bits(full["features"][perm.numpy()]))
    assert np.array_equal(_bits(p["grads"]["features"]), _bits(full["grads"]["features"][:, perm.numpy()]))


# ---- 5. composition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "posed"])
def test_composition_with_the_other_backwards(hip_device, exact_mode, name):
    cam, cloud, degree, bg = fr.case(name)
    H, W = cam.image_height, cam.image_width
    r, n, d = fr.reference(name), rn.reference(name), dr.reference(name, "ndc")
    feats = r["feats"]
    frag = torch.from_numpy(np.array(r["fragile"]) | np.array(n["fragile"]) | np.array(d["fragile"]))
    gf, gn, gd = r["G"].clone(), n["G"].clone(), d["G"] * 1000.0      # (the "ndc" distortion is small: brought to the others' size)
    for g in (gf, gn, gd):                                            # zero on the pixels any reference calls fragile
        g[:, frag] = 0.0
    gc = synthetic.upstream_grad(H, W)
    # float64: the terms' gradients add
    f64, _ = fr.grads64(cloud, cam, feats, gf.numpy())
    c64, _, _, _, _ = rn.grads64(cloud, cam, degree, bg, np.zeros((3, H, W)), gc=gc)
    cn64, _, _, _, _ = rn.grads64(cloud, cam, degree, bg, gn.numpy(), gc=gc)
    d64, _, _, _ = dr.grads64(cloud, cam, degree, bg, dr.coefficients("ndc"), gd.numpy())
    two64 = dict({k: c64[k] + f64[k] for k in GEO}, sh=c64["sh"], features=f64["features"])
    all64 = dict({k: cn64[k] + d64[k] + f64[k] for k in GEO}, sh=cn64["sh"], features=f64["features"])
    run = lambda **kw: _run(cloud, cam, degree, bg, hip_device, **kw)
    colour = run(gc=gc)
    alone = run(feats=feats, gf=gf)
    two = run(feats=feats, gc=gc, gf=gf)
    every = run(feats=feats, gc=gc, gf=gf, gn=gn, gd=gd, normals=True, distortion=True)
    for label, got, want in (("colour + features", two, two64), ("colour + normals + distortion + features", every, all64)):
        g = {REF_KEY[k]: v for k, v in got["grads"].items()}
        for k in GEO + ["sh", "features"]:
            print(name, label, k, "err %.2e of max %.3e" % (np.abs(g[k].reshape(want[k].shape) - want[k]).max() / np.abs(want[k]).max(),
                                                            np.abs(want[k]).max()))
        hp.compare_grads(g, want, names=GEO + ["sh", "features"])
    for k in GEO:                                                     # the term is not lost against the colour's
        kk = [m for m in NAMES if REF_KEY[m] == k][0]
        assert np.abs(alone["grads"][kk]).max() > 0.01 * np.abs(colour["grads"][kk]).max(), k
    # fused gradient accumulation on: the same bits; two runs: the same bits, forward and backward
    for base, kw in ((two, dict()), (every, dict(gn=gn, gd=gd, normals=True, distortion=True))):
        fused = run(feats=feats, gc=gc, gf=gf, fused=True, **kw)
        again = run(feats=feats, gc=gc, gf=gf, **kw)
        assert np.array_equal(_bits(again["features"]), _bits(base["features"]))
        for k in NAMES:
            differ = _bits(fused["grads"][k]) != _bits(base["grads"][k])
            print(name, k, "fused against unfused:", int(differ.sum()), "words differ, by",
                  float(np.abs(fused["grads"][k] - base["grads"][k]).max()), "at most")
            assert np.array_equal(_bits(again["grads"][k]), _bits(base["grads"][k])), k
            assert np.array_equal(_bits(fused["grads"][k]), _bits(base["grads"][k])), k
    # an unused feature output (with unused alpha, median, normals and distortion outputs next to it): the colour gradients' bits,
    # a zero gradient for the table, and every other output's bits
    unused = run(feats=feats, gc=gc, alpha=True, median=True, normals=True, distortion=True)
    others = run(gc=gc, alpha=True, median=True, normals=True, distortion=True)
    for k in ("color", "depth", "radii", "alpha", "median_depth", "median_ids", "normals", "distortion"):
        assert np.array_equal(unused[k], others[k]), k
    for k in NAMES[:-1]:
        assert np.array_equal(_bits(unused["grads"][k]), _bits(colour["grads"][k])), k
    assert not unused["grads"]["features"].any()
    assert np.array_equal(_bits(unused["features"]), _bits(two["features"]))


def test_an_unused_feature_output_launches_nothing(hip_device, exact_mode, monkeypatch):
    from luciddreamer_amd import _C
    cam, cloud, degree, bg = fr.case("thin")

    def boom(*a, **k):
        raise AssertionError("lr_render_features_backward was called for an unused output")
    monkeypatch.setattr(_C, "render_features_backward", boom)
    out = _run(cloud, cam, degree, bg, hip_device, feats=fr.features_of("thin", 5), gc=synthetic.upstream_grad(cam.image_height, cam.image_width))
    assert out["grads"]["means3D"].any() and not out["grads"]["features"].any()


# ---- 6. the output order --------------------------------------------------------------------------------------------------------
def test_output_order_with_every_optional_output(hip_device):
    """colour, radii, depth, alpha, median_depth, median_ids, normals, feature_map, distortion (asserted inside _run), through both
    entry points, render / render_raw and the installed render."""
    from types import SimpleNamespace
    from luciddreamer_amd import dropin
    from luciddreamer_amd.gaussian_renderer import render, render_raw
    from luciddreamer_amd.rasterizer import rasterize_gaussians_raw
    cam, cloud, degree, bg = fr.case("thin")
    H, W = cam.image_height, cam.image_width
    C = K + 3
    feats = fr.features_of("thin", C)
    out = _run(cloud, cam, degree, bg, hip_device, feats=feats, alpha=True, median=True, normals=True, distortion=True)
    only = _run(cloud, cam, degree, bg, hip_device, feats=feats)
    assert np.array_equal(_bits(out["features"]), _bits(only["features"])) and out["features"].any()
    pc = _raw_cloud(cloud, degree, hip_device)
    rs = _settings(cam, bg, degree, hip_device)
    table = feats.to(hip_device)
    raw = rasterize_gaussians_raw(pc._xyz, torch.zeros_like(pc._xyz), pc._features_dc, pc._features_rest, pc._opacity, pc._scaling,
                                  pc._rotation, rs, return_alpha=True, return_median=True, return_distortion=True, return_normals=True,
                                  features=table)
    assert [tuple(t.shape) for t in raw[3:]] == [(1, H, W), (1, H, W), (H, W), (3, H, W), (C, H, W), (1, H, W)]
    every = dict(return_alpha=True, return_median=True, return_distortion=True, return_normals=True, features=table)
    pkg = render_raw(cam.to(hip_device), pc, bg_color=bg.to(hip_device), **every)
    assert torch.equal(pkg["features"], raw[7]) and torch.equal(pkg["normals"], raw[6]) and torch.equal(pkg["distortion"], raw[8])
    assert torch.equal(pkg["alpha"], raw[3]) and torch.equal(pkg["median_ids"], raw[5])
    act = render(cam.to(hip_device), pc, bg_color=bg.to(hip_device), **every)
    assert act["features"].shape == (C, H, W) and "features" not in render(cam.to(hip_device), pc, bg_color=bg.to(hip_device))
    assert act["features"].any() and float((act["features"].detach() - pkg["features"].detach()).abs().max()) <= 1e-3     # (two routes to the activations)
    b = render_raw(cam.to(hip_device), pc, bg_color=bg.to(hip_device), render_only=True, features=table)
    assert set(b) == {"render", "depth", "features"} and torch.equal(b["features"], pkg["features"])

    def reference_render(*args, **kw):
        raise AssertionError("the reference's render cannot return a feature map")
    ns = SimpleNamespace(render=reference_render)
    opt = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    h = dropin.install(ns, None, None, losses=False, adam=False, stats=False)
    try:
        got = ns.render(cam.to(hip_device), pc, opt, bg.to(hip_device), **every)
        over = ns.render(cam.to(hip_device), pc, opt, bg.to(hip_device), override_color=torch.ones_like(pc._xyz), features=table)
    finally:
        dropin.uninstall(h)
    assert torch.equal(got["features"], pkg["features"]) and torch.equal(got["distortion"], pkg["distortion"])
    assert over["features"].shape == (C, H, W) and over["features"].any()


# ---- 7. the armed fused optimizer step ----------------------------------------------------------------------------------------
def test_armed_fused_step_takes_the_feature_gradient(hip_device):
    """The armed FusedAdam (raw node's no-zero-fill backward + masked step) with a colour + features loss: the same parameter
    bits as backward + step(), and the same gradient for the table (a torch leaf outside the armed set)."""
    import torch.nn as nn
    from luciddreamer_amd import cameras
    from luciddreamer_amd.gaussian_renderer import render_raw
    from tests.test_gpu_optim import _adam_for, _two_clouds
    params = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    W, H, P, C = 144, 96, 3000, K + 3
    a, b = _two_clouds(P, hip_device)
    for cl in (a, b):
        for n in params:
            setattr(cl, n, nn.Parameter(getattr(cl, n).detach()))
    opt_a, opt_b = _adam_for(a), _adam_for(b)
    cams = [c.to(hip_device) for c in cameras.rotate360_path(W, H, n_views=12)]
    bg = torch.zeros(3, device=hip_device)
    gen = torch.Generator().manual_seed(13)
    t0 = (2.0 * torch.rand(P, C, generator=gen) - 1.0).to(hip_device)
    ta, tb = t0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
    moved = False
    for it in range(3):
        cam = cams[(5 * it) % 12]
        g = torch.randn(3, H, W, generator=gen).to(hip_device)
        gf = torch.randn(C, H, W, generator=gen).to(hip_device)
        pa = render_raw(cam, a, bg_color=bg, features=ta)
        ((pa["render"] * g).sum() + (pa["features"] * gf).sum()).backward()
        opt_a.step()
        opt_a.zero_grad(set_to_none=True)
        assert opt_b.arm_fused_backward()
        pb = render_raw(cam, b, bg_color=bg, features=tb)
        ((pb["render"] * g).sum() + (pb["features"] * gf).sum()).backward()
        assert all(getattr(b, n).grad is None for n in params)
        opt_b.step()
        opt_b.zero_grad(set_to_none=True)
        moved |= bool(pa["features"].any())
        assert torch.equal(pa["features"], pb["features"]), it
        assert torch.equal(ta.grad, tb.grad) and ta.grad.any(), it
        ta.grad = tb.grad = None
        for n in params:
            assert torch.equal(getattr(a, n), getattr(b, n)), (it, n)
    assert moved


def test_example_loop_trains_a_feature_table(hip_device):
    """examples/train_loop.py --feature-channels: the term is printed, is in the loss from the first iteration on and moves."""
    import importlib.util
    import math
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_loop_example_features_gpu", os.path.join(root, "examples", "train_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    small = dict(gaussians=2000, iters=30, resolution="64x64", log=1)
    plain, _ = mod.train(mod.default_args(**small), log=lambda s: None)
    losses, _ = mod.train(mod.default_args(feature_channels=K + 3, **small), log=lines.append)
    assert len(losses) == 30 and all(math.isfinite(l) for _, l, _ in losses)
    assert losses[0][1] > plain[0][1] and len({n for _, _, n in losses}) == 1          # the term is there; the set stays fixed
    terms = [float(m.group(1)) for m in (re.search(r"feature L1 ([0-9.]+)", ln) for ln in lines) if m]
    assert len(terms) == 30 and all(math.isfinite(t) for t in terms)
    # the table starts at zero, so the first term is the target's own mean magnitude; a random view per iteration makes the curve
    # noisy, but the table learns: the term falls below its start
    assert min(terms[1:]) < terms[0] and len(set(terms)) > 10
    with pytest.raises(SystemExit):
        mod.train(mod.default_args(feature_channels=4, multi_view=2, **small), log=lambda s: None)


# ---- 8. anti-aliasing ---------------------------------------------------------------------------------------------------------
def test_gradients_with_antialiasing_on(hip_device, exact_mode):
    """The blend sees opacity x coef (tests/aa_ref.py): the reference is fed the compensated opacity, whose own derivative reaches
    the scales."""
    cam, cloud, degree, bg = fr.case("sparse")
    r = fr.aa_reference("sparse")
    plain = fr.reference("sparse")
    assert np.abs(r["leaf"]["scales"] - plain["leaf"]["scales"]).max() > 100 * hp.GRAD_RTOL * np.abs(plain["leaf"]["scales"]).max()
    config.set_antialiasing(True)
    try:
        got = _run(cloud, cam, degree, bg, hip_device, feats=r["feats"], gf=r["G"])
    finally:
        config.set_antialiasing(False)
    ok = ~r["fragile"]
    assert np.abs(got["features"].astype(np.float64) - r["F64"])[:, ok].max() <= FWD_BAR * fr.FWD_ERR["sparse"]
    g = {REF_KEY[k]: v for k, v in got["grads"].items()}
    hp.compare_grads(g, r["leaf"], names=GEO + ["features"])


# ---- 9. edges of the C ABI ----------------------------------------------------------------------------------------------------
def test_c_abi_edges(hip_device):
    from luciddreamer_amd import _C, cameras
    cam, cloud, _, _ = fr.case("sparse")
    H, W, P = cam.image_height, cam.image_width, cloud["means3D"].shape[0]
    C = K + 3
    dev = hip_device
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rs = _settings(cam, torch.zeros(3), 3, dev)
    feats = fr.features_of("sparse", C).to(dev)
    inputs = dict(means3D=cloud["means3D"].to(dev), scales=cloud["scales"].to(dev), rotations=cloud["rotations"].to(dev))
    exact = _forward_c_abi(cloud, cam, dev, 0)
    f0 = _C.render_features(exact[4], exact[5], exact[6], feats, rs)
    assert f0.any() and f0.shape == (C, H, W)
    # a capacity that holds the view: the exact forward's bits
    cap = 4 * int(exact[0]) + 1024
    roomy = _forward_c_abi(cloud, cam, dev, cap)
    f1 = _C.render_features(roomy[4], roomy[5], roomy[6], feats, rs, binning_capacity=cap)
    assert torch.equal(f0, f1)
    # an async forward whose binning capacity is too small: zeros, rc 0, the overflow is lr_check's to report; the backward adds nothing
    over = _forward_c_abi(cloud, cam, dev, 100)
    fz = _C.render_features(over[4], over[5], over[6], feats, rs, binning_capacity=100)
    assert not fz.any()
    with pytest.raises(RuntimeError, match="capacity"):
        _C.check(over[4])
    G = torch.ones(C, H, W, device=dev)
    shapes = (("means2D", (P, 3)), ("opacity", (P, 1)), ("means3D", (P, 3)), ("scales", (P, 3)), ("rotations", (P, 4)), ("features", (P, C)))
    acc = {k: torch.full(s, 3.0, device=dev) for k, s in shapes}
    _C.render_features_backward(over[4], over[5], over[6], G, fz, feats, over[3], rs, slots=1, binning_capacity=100, accumulate_into=acc,
                                **inputs)
    assert all(bool((t == 3.0).all()) for t in acc.values())
    o = _C.render_features_backward(over[4], over[5], over[6], G, fz, feats, over[3], rs, slots=1, binning_capacity=100, **inputs)
    assert all(not t.any() for t in o.values() if t is not None)
    # write mode and accumulate mode of a view that holds: the same gradients, in exact and in async mode
    w = _C.render_features_backward(exact[4], exact[5], exact[6], G, f0, feats, exact[3], rs, slots=int(exact[0]), **inputs)
    acc = {k: torch.zeros_like(t) for k, t in w.items() if t is not None}
    _C.render_features_backward(exact[4], exact[5], exact[6], G, f0, feats, exact[3], rs, slots=int(exact[0]), accumulate_into=acc, **inputs)
    w3 = _C.render_features_backward(roomy[4], roomy[5], roomy[6], G, f1, feats, roomy[3], rs, slots=1, binning_capacity=cap, **inputs)
    assert w["means3D"].any() and w["features"].any() and w["cov3D"] is None
    for k, t in acc.items():
        assert torch.equal(t, w[k]), k
        assert torch.equal(w3[k], w[k]), k
    _C.check(exact[4])                                   # the workspace held the view: nothing to report
    # P = 0: zeros, no buffer read (none is given); the backward has nothing to do
    fz = torch.ones(C, H, W, device=dev)
    a = _lib.FeatureRenderArgs(view=_lib.View(P=0, width=W, height=H), channels=C, out_features=fz.data_ptr(), stream=stream)
    assert L.lr_render_features(a) == 0
    torch.cuda.synchronize()
    assert not fz.any()
    assert L.lr_render_features_backward(_lib.FeatureRenderBackwardArgs(view=_lib.View(P=0, width=W, height=H), channels=C)) == 0
    # a 1 x 1 and a 17 x 16 image: a tile with one pixel, and a second tile column one pixel wide
    for (w_, h_) in ((1, 1), (17, 16)):
        c = cameras.identity_camera(w_, h_)
        f = _forward_c_abi(cloud, c, dev, 0)
        rs_ = _settings(c, torch.zeros(3), 3, dev)
        ff = _C.render_features(f[4], f[5], f[6], feats, rs_)
        st = hp.run_oracle(cloud, c, 3, torch.zeros(3))
        F32, layers32, fragile = fr.walk32(st["res"].stage(), w_, h_, feats.cpu().numpy())
        assert ff.shape == (C, h_, w_) and (layers32.max() > 0 or (w_, h_) == (1, 1))
        err = np.abs(ff.cpu().numpy() - F32)[:, ~fragile].max() if (~fragile).any() else 0.0
        print("%d x %d: err against the float32 walk %.3e" % (w_, h_, err))
        assert err <= FWD_BAR * max(fr.FWD_ERR.values())
        o = _C.render_features_backward(f[4], f[5], f[6], torch.ones(C, h_, w_, device=dev), ff, feats, f[3], rs_, slots=int(f[0]),
                                        **inputs)
        assert all(bool(torch.isfinite(t).all()) for t in o.values() if t is not None) and (o["features"].any() or layers32.max() == 0)
    # a wrong struct_bytes and a missing required pointer, with everything else in place
    a = _lib.FeatureRenderArgs(view=_lib.View(P=P, width=W, height=H), geom_buffer=exact[4].data_ptr(),
                               binning_buffer=exact[5].data_ptr(), image_buffer=exact[6].data_ptr(), out_features=fz.data_ptr(),
                               channels=C, stream=stream)
    assert L.lr_render_features(a) == _lib.LR_ERR_INVALID_ARG and b"required" in L.lr_last_error()
    a.struct_bytes = ctypes.sizeof(_lib.FeatureRenderArgs) - 8
    assert L.lr_render_features(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    torch.cuda.synchronize()
