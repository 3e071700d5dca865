"""Anti-aliased splatting on the GPU (config.set_antialiasing -> lr_set_antialiasing).

With the setting on, preprocess stores `opacity * coef` in every record (coef = sqrt(max(0.000025, det0 / det)), tests/aa_ref.py)
and nothing else changes, so an anti-aliased render IS the plain renderer on pre-scaled opacities: the forward is checked against
the CPU oracle fed `opacity * coef32` and, bit for bit, against the GPU's own plain render of them; the gradients against a
COMPOSED expectation -- the oracle's backward on the pre-scaled opacities (dL/d(record opacity) and the geometry gradients at
fixed coefficient) plus the coefficient's own derivative from float64 autograd of aa_ref.coef64.  tests/test_aa_cpu.py checks
on the CPU that the inputs used here are fit for that (coef32 within 1e-5 of coef64, flagged pixels under the cap)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, cameras, config, synthetic
from tests import aa_cases, aa_ref, grad_oracle, helpers as hp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES_SH = ["means2D", "opacity", "means3D", "sh", "scales", "rotations"]
NAMES_PRE = ["means2D", "colors", "opacity", "means3D", "cov3D"]


@pytest.fixture
def aa_on():
    config.set_antialiasing(True)
    yield
    config.set_antialiasing(False)


@pytest.fixture
def exact_mode():
    """Bit comparisons between calls: every forward in exact mode (async mode's binning bound can pick another shape)."""
    config.set_async(False)
    yield
    config.set_async(True)
    config.reset()


def _cov3d(cloud):
    return aa_ref.cov3d64(cloud["scales"].double(), cloud["rotations"].double()).float()


def _coef_grad_terms(cam, cloud, weight, scale_modifier=1.0, cov3D_precomp=None):
    """d/d(geometry) of sum_i weight_i coef64_i: the part of the anti-aliased gradient that the oracle's backward at fixed
    coefficient does not hold (weight = dL/d(record opacity) * opacity).  float64 autograd of tests/aa_ref.coef64."""
    tfx, tfy = hp.tan_fov(cam)
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    m = leaf(cloud["means3D"])
    if cov3D_precomp is not None:
        geo = dict(cov3D=leaf(cov3D_precomp))
        c = aa_ref.coef64(m, cam.world_view_transform, tfx, tfy, cam.image_width, cam.image_height, cov3D_precomp=geo["cov3D"])
    else:
        # the reference's backward differentiates with respect to the MODIFIED scale mod * s (backward.cu:278-341 forms
        # dL/dscale from s = mod * scale and never multiplies by mod; oracle/raster_oracle.c computeCov3D_bwd and the kernels
        # keep that), and the coefficient's term rides the same chain: the leaf is mod * s
        geo = dict(scales=leaf(cloud["scales"].double() * scale_modifier), rotations=leaf(cloud["rotations"]))
        c = aa_ref.coef64(m, cam.world_view_transform, tfx, tfy, cam.image_width, cam.image_height, geo["scales"],
                          geo["rotations"], 1.0)
    (torch.from_numpy(np.asarray(weight, np.float64)) * c).sum().backward()
    out = {k: v.grad.numpy() for k, v in geo.items()}
    out["means3D"] = m.grad.numpy()
    return out


def _compose(ref_grads, cam, cloud, coef, scale_modifier=1.0, cov3D_precomp=None):
    """Expected anti-aliased gradients from the fixed-coefficient ones (any reference's, numpy, the oracle's naming)."""
    g_rec = np.asarray(ref_grads["opacity"], np.float64).reshape(-1)
    op = cloud["opacities"].numpy().astype(np.float64).reshape(-1)
    exp = {k: np.array(v, dtype=np.float64) for k, v in ref_grads.items()}
    exp["opacity"] = (g_rec * coef.astype(np.float64)).reshape(np.shape(ref_grads["opacity"]))
    for k, v in _coef_grad_terms(cam, cloud, g_rec * op, scale_modifier, cov3D_precomp).items():
        exp[k] = exp[k] + v.reshape(exp[k].shape)
    return {k: v.astype(np.float32) for k, v in exp.items()}


# ---- 1. off is off -----------------------------------------------------------------------------------------------------------
def test_off_is_bit_equal_to_a_process_that_never_touched_the_setting(hip_device, tmp_path):
    out = tmp_path / "untouched.npz"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-m", "tests.aa_cases", str(out)], cwd=ROOT, env=env, check=True, timeout=600)
    want = np.load(out)
    config.set_antialiasing(True)
    try:
        on = aa_cases.render_off_case(hip_device)
    finally:
        config.set_antialiasing(False)
    off = aa_cases.render_off_case(hip_device)
    for k in want.files:
        assert np.array_equal(off[k], want[k]), k
    assert np.array_equal(on["radii"], want["radii"])
    assert not np.array_equal(on["color"], want["color"])           # and on is not off


# ---- 2. forward against the oracle on pre-scaled opacities ----------------------------------------------------------------
FWD_VARIANTS = [
    # case, preprocess kernel, colors_precomp, cov3D_precomp, scale_modifier, strict
    (0, 0, False, False, 1.0, False), (0, 1, False, False, 1.0, False),
    (1, 0, False, False, 1.0, False), (1, 1, False, False, 1.0, False),
    (1, 0, True, True, 1.0, False), (1, 1, True, True, 1.0, False),
    (0, 0, True, False, 1.7, False), (1, 1, False, False, 0.6, False),
    (1, 0, False, False, 1.0, True), (0, 1, False, True, 1.0, True),
]


@pytest.mark.parametrize("case,pre,precol,precov,modifier,strict", FWD_VARIANTS)
def test_forward_matches_oracle_on_prescaled_opacities(hip_device, case, pre, precol, precov, modifier, strict):
    cam, cloud = aa_cases.box_case(*aa_cases.FORWARD_CASES[case])
    P = cloud["means3D"].shape[0]
    bg = torch.tensor([0.0, 0.1, 0.2])
    cov = _cov3d(cloud) if precov else None
    cols = torch.rand(P, 3, generator=torch.Generator().manual_seed(5)) if precol else None
    coef = aa_cases.coef_of(cam, cloud, modifier, cov)
    ref = hp.run_oracle(aa_cases.prescaled(cloud, coef), cam, 2, bg, colors_precomp=cols, cov3D_precomp=cov,
                        scale_modifier=modifier)
    vis = ref["radii"] > 0
    assert float(coef[vis].min()) < 0.9                         # the coefficient matters on this input
    _lib.tune_set("preprocess", pre)
    config.set_strict_parity(strict)
    config.set_antialiasing(True)
    try:
        hip = hp.run_hip(cloud, cam, 2, bg, hip_device, colors_precomp=cols, cov3D_precomp=cov, scale_modifier=modifier)
    finally:
        config.set_antialiasing(False)
        config.set_strict_parity(False)
        _lib.tune_set("preprocess", -1)
    fig = hp.compare_forward(hip, ref)                          # radii exact, colour 1e-5 off the flagged pixels, depth 1e-5 rel
    print(fig)
    # ... and the plain render of the same inputs is somewhere else
    plain = hp.run_hip(cloud, cam, 2, bg, hip_device, colors_precomp=cols, cov3D_precomp=cov, scale_modifier=modifier)
    assert np.abs(plain["color"] - hip["color"]).max() > 1e-3


# ---- 3. the same kernels: AA on with opacity == AA off with opacity * coef32, bit for bit ---------------------------------
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("case", [0, 1])
def test_antialiased_render_is_the_plain_render_of_prescaled_opacities_bit_for_bit(hip_device, exact_mode, case, pre):
    """The record's opacity is the only thing that differs, and it is one correctly rounded division, square root and product
    of values the restatement forms bit for bit (tests/test_aa_cpu.py): images, radii and every gradient that does not pass
    through the coefficient (means2D, SH) are the same bits."""
    cam, cloud = aa_cases.grad_case(case)
    H, W = cam.image_height, cam.image_width
    bg = torch.tensor([0.0, 0.1, 0.2])
    g = synthetic.upstream_grad(H, W)
    full = aa_cases.coef_of(cam, cloud, full=True)
    _lib.tune_set("preprocess", pre)
    try:
        config.set_antialiasing(True)
        try:
            on = hp.run_hip(cloud, cam, 3, bg, hip_device, g)
        finally:
            config.set_antialiasing(False)
        off = hp.run_hip(aa_cases.prescaled(cloud, full["coef"]), cam, 3, bg, hip_device, g)
    finally:
        _lib.tune_set("preprocess", -1)
    for k in ("radii", "color", "depth"):
        assert np.array_equal(on[k], off[k]), (k, float(np.abs(on[k] - off[k]).max()))
    for k in ("means2D", "sh"):
        assert np.array_equal(on["grads"][k], off["grads"][k]), k
    # dL/dopacity = g coef against the same g.  Not asserted bit for bit: the backward recomputes the coefficient from a
    # covariance it forms with FMA contraction (csrc/gauss_bwd.hip is not a contraction-free translation unit), the forward's
    # and coef32 are contraction-free -- the gradient bar of helpers.compare_grads applies
    vis = on["radii"] > 0
    want = off["grads"]["opacity"][:, 0] * full["coef"]
    err = np.abs(on["grads"]["opacity"][:, 0] - want)[vis].max()
    print(f"dL/dopacity against g * coef32: max error {err:.3e} of {np.abs(want).max():.3e}")
    assert err <= hp.GRAD_RTOL * np.abs(want).max()
    # clamped Gaussians (rho <= floor): the coefficient is a constant there, so the geometry gradient is the fixed-coefficient
    # one: the kernel's added term is exactly zero, and what is left differs from the plain kernel's row by the rounding of
    # two instantiations of the same expressions at most
    cl = vis & (full["rho"] <= np.float32(aa_ref.RHO_FLOOR)) & (np.abs(off["grads"]["opacity"][:, 0]) > 0)
    assert int(cl.sum()) >= 4, int(cl.sum())
    for k in ("means3D", "scales", "rotations"):
        d = np.abs(on["grads"][k][cl] - off["grads"][k][cl]).max()
        print(f"clamped rows, {k}: max |AA - fixed coefficient| = {d:.3e} over {int(cl.sum())} rows, tensor max "
              f"{np.abs(off['grads'][k]).max():.3e}, bit-equal {np.array_equal(on['grads'][k][cl], off['grads'][k][cl])}")
        assert d <= hp.GRAD_RTOL * np.abs(off["grads"][k]).max(), k
    # and elsewhere the coefficient's derivative is really there
    live = vis & ~cl & (full["rho"] < 0.5)
    assert np.abs(on["grads"]["scales"][live] - off["grads"]["scales"][live]).max() > 1e-3 * np.abs(off["grads"]["scales"]).max()


# ---- 4. gradients against the composed expectation ---------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("case", [0, 1])
def test_gradients_match_the_composed_expectation(hip_device, case, strict):
    cam, cloud = aa_cases.grad_case(case)
    H, W = cam.image_height, cam.image_width
    P = cloud["means3D"].shape[0]
    bg = torch.tensor([0.0, 0.1, 0.2])
    g = synthetic.upstream_grad(H, W)
    coef = aa_cases.coef_of(cam, cloud)
    ref = hp.run_oracle(aa_cases.prescaled(cloud, coef), cam, 3, bg, g)
    exp = dict(ref)
    exp["grads"] = _compose(ref["grads"], cam, cloud, coef)
    config.set_strict_parity(strict)
    config.set_antialiasing(True)
    try:
        hip = hp.run_hip(cloud, cam, 3, bg, hip_device, g)
    finally:
        config.set_antialiasing(False)
        config.set_strict_parity(False)
    hp.compare_forward(hip, ref)
    fig = hp.compare_grads(hip["grads"], exp["grads"], names=NAMES_SH)
    print({k: f"{e / s:.2e}" for k, (e, s) in fig.items()})
    print(hp.compare_grads_by_row(hip, exp, P))
    # the composed part is a real share of the expectation (the test would not notice a missing term otherwise)
    for k in ("scales", "rotations"):
        share = np.abs(exp["grads"][k] - ref["grads"][k]).max() / np.abs(exp["grads"][k]).max()
        assert share > 10 * hp.GRAD_RTOL, (k, share)


def test_gradients_with_precomputed_covariance_and_colours(hip_device, aa_on):
    cam, cloud = aa_cases.grad_case(1)
    H, W = cam.image_height, cam.image_width
    P = cloud["means3D"].shape[0]
    bg = torch.zeros(3)
    g = synthetic.upstream_grad(H, W)
    cov = _cov3d(cloud)
    cols = torch.rand(P, 3, generator=torch.Generator().manual_seed(5))
    coef = aa_cases.coef_of(cam, cloud, cov3D_precomp=cov)
    ref = hp.run_oracle(aa_cases.prescaled(cloud, coef), cam, 0, bg, g, colors_precomp=cols, cov3D_precomp=cov)
    exp = _compose({k: ref["grads"][k] for k in NAMES_PRE}, cam, cloud, coef, cov3D_precomp=cov)
    hip = hp.run_hip(cloud, cam, 0, bg, hip_device, g, colors_precomp=cols, cov3D_precomp=cov)
    hp.compare_forward(hip, ref)
    print(hp.compare_grads(hip["grads"], exp, names=NAMES_PRE))
    assert np.abs(exp["cov3D"] - ref["grads"]["cov3D"]).max() > 10 * hp.GRAD_RTOL * np.abs(exp["cov3D"]).max()


def test_gradients_with_a_scale_modifier(hip_device, aa_on):
    cam, cloud = aa_cases.grad_case(0)
    H, W = cam.image_height, cam.image_width
    bg = torch.zeros(3)
    g = synthetic.upstream_grad(H, W)
    coef = aa_cases.coef_of(cam, cloud, 0.6)
    ref = hp.run_oracle(aa_cases.prescaled(cloud, coef), cam, 2, bg, g, scale_modifier=0.6)
    exp = _compose(ref["grads"], cam, cloud, coef, scale_modifier=0.6)
    hip = hp.run_hip(cloud, cam, 2, bg, hip_device, g, scale_modifier=0.6)
    hp.compare_forward(hip, ref)
    print(hp.compare_grads(hip["grads"], exp, names=NAMES_SH))


# ---- 5. the raw path -----------------------------------------------------------------------------------------------------------
def _pc(cloud, device, degree):
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    c = {k: v.to(device) for k, v in cloud.items()}
    gen = torch.Generator().manual_seed(5)               # un-normalised quaternions: the normalisation Jacobian is exercised
    rot = c["rotations"] * (0.5 + 1.5 * torch.rand(c["rotations"].shape[0], 1, generator=gen).to(device))
    return GaussianCloud(c["means3D"], c["scales"], rot, c["opacities"], c["shs"], active_sh_degree=degree)


RAW_PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


@pytest.mark.parametrize("degree", [3, 0])
def test_raw_path_matches_the_activated_path_under_antialiasing(hip_device, aa_on, degree):
    """rasterize_gaussians_raw under AA against rasterize_gaussians under AA on torch's own activations, gradients chained
    through them by autograd: the bars of tests/test_gpu_raw.py."""
    from luciddreamer_amd.gaussian_renderer import render, render_raw
    cam, cloud = aa_cases.grad_case(1)
    H, W = cam.image_height, cam.image_width
    cam = cam.to(hip_device)
    pc = _pc(cloud, hip_device, degree)
    bg = torch.tensor([0.2, 0.1, 0.3], device=hip_device)
    gcol = synthetic.upstream_grad(H, W, seed=3).to(hip_device)
    grads = lambda: {n: getattr(pc, n).grad.detach().cpu().numpy() for n in RAW_PARAMS if getattr(pc, n).grad is not None}
    out_a = render(cam, pc, bg_color=bg)
    (out_a["render"] * gcol).sum().backward()
    g_a, vs_a = grads(), out_a["viewspace_points"].grad.detach().cpu().numpy()
    for p in pc.parameters():
        p.grad = None
    out_r = render_raw(cam, pc, bg_color=bg)
    (out_r["render"] * gcol).sum().backward()
    g_r, vs_r = grads(), out_r["viewspace_points"].grad.detach().cpu().numpy()
    assert (out_a["radii"] == out_r["radii"]).float().mean().item() >= 0.999
    cerr = (out_a["render"] - out_r["render"]).abs().max().item()
    derr = (out_a["depth"] - out_r["depth"]).abs().max().item()
    assert cerr <= 2e-5 and derr <= 2e-4, (cerr, derr)
    hp.compare_grads({"vs": vs_r}, {"vs": vs_a}, names=("vs",), rtol=2e-4)
    for n in g_a:
        if g_a[n].size == 0 or not np.any(g_a[n]):
            continue
        hp.compare_grads({n: g_r[n]}, {n: g_a[n]}, names=(n,), rtol=2e-4)
    # the anti-aliased raw render is not the plain raw render
    config.set_antialiasing(False)
    with torch.no_grad():
        plain = render_raw(cam, pc, bg_color=bg)["render"]
    assert (plain - out_r["render"]).abs().max().item() > 1e-3


# ---- 6. depth gradient and alpha output under AA --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["depth", "alpha", "depth_alpha"])
def test_depth_and_alpha_modes_under_antialiasing(hip_device, aa_on, mode):
    """The float64 references of the depth and alpha modes (tests/grad_oracle.py) on the pre-scaled opacities give dL/d(record
    opacity) and the fixed-coefficient geometry gradients; the coefficient's derivative is composed onto them as above."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    cam, cloud = aa_cases.grad_case(1)
    H, W = cam.image_height, cam.image_width
    P = cloud["means3D"].shape[0]
    bg = torch.zeros(3)
    img = lambda seed: torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed))
    gc = synthetic.upstream_grad(H, W)
    gd = img(22) if "depth" in mode else None
    ga = img(21) if "alpha" in mode else None
    coef = aa_cases.coef_of(cam, cloud)
    pre = aa_cases.prescaled(cloud, coef)
    tfx, tfy = hp.tan_fov(cam)
    # float64 reference on the pre-scaled opacities
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    r = {k: leaf(pre[k]) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    m2r = torch.zeros(P, 3, dtype=torch.float64, requires_grad=True)
    col, dep, alpha, _ = grad_oracle.render(r["means3D"], r["opacities"], cam.world_view_transform, cam.full_proj_transform,
                                            cam.camera_center, tfx, tfy, H, W, bg, scales=r["scales"], rotations=r["rotations"],
                                            shs=r["shs"], degree=3, means2D=m2r, alpha=True)
    loss = (col * gc.double()).sum()
    if gd is not None:
        loss = loss + (dep * gd.double()).sum()
    if ga is not None:
        loss = loss + (alpha * ga.double()).sum()
    loss.backward()
    fixed = dict(means2D=m2r.grad.numpy(), opacity=r["opacities"].grad.numpy(), means3D=r["means3D"].grad.numpy(),
                 sh=r["shs"].grad.numpy(), scales=r["scales"].grad.numpy(), rotations=r["rotations"].grad.numpy())
    exp = _compose(fixed, cam, cloud, coef)
    # the GPU
    dev = hip_device
    d = lambda t: t.detach().to(dev).requires_grad_(True)
    h = {k: d(cloud[k]) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    c = cam.to(dev)
    rs = GaussianRasterizationSettings(H, W, tfx, tfy, bg.to(dev), 1.0, c.world_view_transform, c.full_proj_transform, 3,
                                       c.camera_center, False, False)
    config.set_depth_gradient("depth" in mode)
    try:
        out = GaussianRasterizer(rs)(means3D=h["means3D"], means2D=m2, opacities=h["opacities"], shs=h["shs"],
                                     scales=h["scales"], rotations=h["rotations"], return_alpha=ga is not None)
        loss = (out[0] * gc.to(dev)).sum()
        if gd is not None:
            loss = loss + (out[2] * gd.to(dev)).sum()
        if ga is not None:
            loss = loss + (out[3] * ga.to(dev)).sum()
        loss.backward()
    finally:
        config.set_depth_gradient(False)
    got = dict(means2D=m2.grad, opacity=h["opacities"].grad, means3D=h["means3D"].grad, sh=h["shs"].grad, scales=h["scales"].grad,
               rotations=h["rotations"].grad)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    fig = hp.compare_grads(got, exp, names=NAMES_SH)
    print({k: f"{e / s:.2e}" for k, (e, s) in fig.items()})


# ---- 7. the multi-view step ----------------------------------------------------------------------------------------------
def test_view_batch_under_antialiasing_equals_the_sum_of_per_view_backwards(hip_device, aa_on):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd import parallel
    P, W, H = 25_000, 256, 160
    cloud = synthetic.make_cloud(P, "band", 6, scale_mult=0.5)
    cams = [c.to(hip_device) for c in cameras.rotate360_path(W, H, n_views=5)]
    g = synthetic.upstream_grad(H, W).to(hip_device)
    bg = torch.tensor([0.1, 0.0, 0.2], device=hip_device)
    leaf = {k: v.to(hip_device).requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros(P, 3, device=hip_device, requires_grad=True)
    for c in cams:
        tfx, tfy = hp.tan_fov(c)
        rs = GaussianRasterizationSettings(H, W, tfx, tfy, bg, 1.0, c.world_view_transform, c.full_proj_transform, 3,
                                           c.camera_center, False, False)
        col, _, _ = GaussianRasterizer(rs)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"], shs=leaf["shs"],
                                           scales=leaf["scales"], rotations=leaf["rotations"])
        col.backward(g)
    ref = {k: v.grad.clone() for k, v in leaf.items()}
    ref["means2D"] = m2d.grad.clone()
    names = {"means3D": "means3D", "means2D": "means2D", "opacity": "opacities", "sh": "shs", "scales": "scales",
             "rotations": "rotations"}
    shapes = {"means3D": (P, 3), "means2D": (P, 3), "opacity": (P, 1), "sh": (P, 16, 3), "scales": (P, 3), "rotations": (P, 4)}
    det = {k: v.detach() for k, v in leaf.items()}
    results = {}
    # the blend shapes pinned, as in the chain-count tests of tests/test_gpu_parity.py: the number of chains is a hint the
    # launchers pick between shapes on, and the shapes agree to float rounding, not to the bit
    _lib.tune_set("blend_quad", 2)
    _lib.tune_set("fwd_pair", 2)
    try:
        for n_streams in (1, 3):
            batch = parallel.ViewBatch(cams, [g] * len(cams), 3, bg, binning_capacity=400_000, n_streams=n_streams)
            acc = {k: torch.zeros(s, device=hip_device) for k, s in shapes.items()}
            with torch.no_grad():
                batch.run(det["means3D"], det["opacities"], det["scales"], det["rotations"], det["shs"], acc)
            batch.check()
            results[n_streams] = acc
            for k, rk in names.items():
                a, b = acc[k].cpu().numpy(), ref[rk].cpu().numpy()
                assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 2e-5 * np.abs(b).max(), (n_streams, k)
    finally:
        _lib.tune_set("blend_quad", -1)
        _lib.tune_set("fwd_pair", -1)
    for k in shapes:
        assert torch.equal(results[1][k], results[3][k]), k
    # the step honoured the setting: the plain step's bucket is somewhere else
    config.set_antialiasing(False)
    acc0 = {k: torch.zeros(s, device=hip_device) for k, s in shapes.items()}
    with torch.no_grad():
        parallel.ViewBatch(cams, [g] * len(cams), 3, bg, binning_capacity=400_000, n_streams=3).run(
            det["means3D"], det["opacities"], det["scales"], det["rotations"], det["shs"], acc0)
    assert float((acc0["scales"] - results[3]["scales"]).abs().max()) > 1e-3 * float(acc0["scales"].abs().max())


# ---- 8. a backward under another setting than its forward raises ----------------------------------------------------------
@pytest.mark.parametrize("node", ["compiled", "python", "raw"])
@pytest.mark.parametrize("forward_on", [True, False])
def test_backward_under_another_setting_raises_before_writing(hip_device, node, forward_on):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd.gaussian_renderer import render_raw
    W, H = 96, 64
    cam, cloud = aa_cases.box_case(2_000, W, H, 1, 1.0)
    dev = hip_device
    config.set_antialiasing(forward_on)
    try:
        if node == "raw":
            pc = _pc(cloud, dev, 1)
            leaves = list(pc.parameters())
            color = render_raw(cam.to(dev), pc, bg_color=torch.zeros(3, device=dev))["render"]
        else:
            leaf = {k: v.to(dev).requires_grad_(True) for k, v in cloud.items()}
            m2 = torch.zeros(2_000, 3, device=dev, requires_grad=True)
            leaves = list(leaf.values()) + [m2]
            tfx, tfy = hp.tan_fov(cam)
            c = cam.to(dev)
            rs = GaussianRasterizationSettings(H, W, tfx, tfy, torch.zeros(3, device=dev), 1.0, c.world_view_transform,
                                               c.full_proj_transform, 1, c.camera_center, False, node == "python")
            color = GaussianRasterizer(rs)(means3D=leaf["means3D"], means2D=m2, opacities=leaf["opacities"], shs=leaf["shs"],
                                           scales=leaf["scales"], rotations=leaf["rotations"])[0]
        config.set_antialiasing(not forward_on)
        with pytest.raises(RuntimeError, match="anti-aliasing"):
            color.sum().backward(retain_graph=True)
        assert all(t.grad is None for t in leaves)
        config.set_antialiasing(forward_on)                 # back under the forward's setting the same node runs
        color.sum().backward()
        assert all(t.grad is not None for t in leaves[:1])
    finally:
        config.set_antialiasing(False)


# ---- 9. what it is for -------------------------------------------------------------------------------------------------------
def test_a_receding_emitter_keeps_its_energy_with_antialiasing(hip_device):
    """One isotropic Gaussian of fixed world size, opacity 0.5, colour 1 on black, at distances where it spans ~4.7 px (sigma
    2 px) down to ~0.5 px (sigma 0.2 px; rho stays above 2e-3, far from the floor).  E(z) = z^2 * sum(pixels) is constant for a
    fixed emitter.  Without the compensation the 0.3 dilation stops the footprint from shrinking and E grows like
    1 + 0.3 / sigma^2; with it E is flat up to what the 3-sigma rectangle, the 1/255 cut and pixel sampling lose."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    W = H = 128
    cam = cameras.identity_camera(W, H)
    tfx, tfy = hp.tan_fov(cam)
    focal = W / (2.0 * tfx)
    z0 = 2.0
    s = 2.0 * z0 / focal                                     # world sigma: 2 px at z0
    c = cam.to(hip_device)
    rs = GaussianRasterizationSettings(H, W, tfx, tfy, torch.zeros(3, device=hip_device), 1.0, c.world_view_transform,
                                       c.full_proj_transform, 0, c.camera_center, False, False)
    spreads = {}
    for on in (False, True):
        config.set_antialiasing(on)
        try:
            E = []
            for k in (1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 6.5, 8.0, 10.0):
                z = z0 * k
                with torch.no_grad():
                    color = GaussianRasterizer(rs)(
                        means3D=torch.tensor([[0.0, 0.0, z]], device=hip_device), means2D=torch.zeros(1, 3, device=hip_device),
                        opacities=torch.tensor([[0.5]], device=hip_device), colors_precomp=torch.ones(1, 3, device=hip_device),
                        scales=torch.full((1, 3), s, device=hip_device),
                        rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=hip_device))[0]
                E.append(z * z * float(color[0].double().sum()))
        finally:
            config.set_antialiasing(False)
        assert min(E) > 0
        spreads[on] = max(E) / min(E)
        print(f"antialiasing {'on' if on else 'off'}: E(z) = {[round(e, 3) for e in E]}, max / min = {spreads[on]:.3f}")
    assert spreads[True] < spreads[False], spreads
