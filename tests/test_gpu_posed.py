"""Posed cameras on the GPU: translated, pitched and rolled views against the references.

Everywhere else in the suite a kernel that is held to a reference sees a camera at the world origin that at most yaws, so
campos, the translation row of the view and projection matrices and the pitch and roll entries of the view matrix never leave
their trivial values in a compared run.  Here every code path that takes a camera runs under the poses of tests/posed_cases.py:
the operator with both preprocess kernels, the raw path, the depth and alpha outputs and their gradients, anti-aliasing, the
multi-view step with each of its options (five different poses in one call) and the layers that unpack a camera object.
tests/test_posed_cases_cpu.py checks on the CPU that every case used here is fit for its comparison (no threshold-fragile
pixel, so gradients are held to the whole-tensor bar) and that each differs by 100 bars or more under the camera bugs it aims at.
Tolerances are the project's own (tests/helpers.py and the files the comparisons are borrowed from).

AbsGS is left out: its float64 reference (tests/absgrad_ref.py) is tied to the identity-camera cases of tests/absgrad_cases.py."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, config, densify, parallel
from tests import helpers as hp, posed_cases as pc
from tests import test_gpu_alpha as al
from tests import test_gpu_depth_grad as dg

pytestmark = pytest.mark.gpu

VIEW_TOL = 2e-5             # a step against per-view runs on the same device (test_view_batch_equals_autograd_accumulation)
RAW_PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
ACC_OF = {"means3D": "means3D", "means2D": "means2D", "opacity": "opacities", "sh": "shs", "scales": "scales",
          "rotations": "rotations"}
PRE_IDS = ["thread_per_gaussian", "pooled"]


@pytest.fixture(autouse=True)
def _restore():
    yield
    for knob in ("preprocess", "pcull", "blend_quad", "fwd_pair"):
        _lib.tune_set(knob, -1)
    config.set_depth_gradient(False)
    config.set_strict_parity(False)
    config.set_antialiasing(False)


def _bg():
    return torch.tensor(pc.BG)


def _report(what, fwd, grads):
    print(f"[posed] {what}: colour {fwd['color_max']:.2e}, depth {fwd['depth_rel_max']:.2e}, gradients " +
          ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in grads.items() if s > 0))


# ---- a. the operator, forward and backward, against the C oracle --------------------------------------------------------------
@pytest.mark.parametrize("pre", [0, 1], ids=PRE_IDS)
@pytest.mark.parametrize("case", list(pc.OP_CASES))
def test_operator_matches_oracle(hip_device, case, pre):
    cam, cloud, degree = pc.make(case)
    ref = pc.reference(case)
    _lib.tune_set("preprocess", pre)
    hip = hp.run_hip(cloud, cam, degree, _bg(), hip_device, pc.upstream(cam))
    fwd = hp.compare_forward(hip, ref)
    assert float(np.abs(ref["grads"]["means3D"]).max()) > 0
    _report(f"{case}, preprocess {pre}", fwd, hp.compare_grads(hip["grads"], ref["grads"], names=pc.NAMES_SH))


@pytest.mark.parametrize("pre", [0, 1], ids=PRE_IDS)
def test_operator_with_own_colours_and_covariances(hip_device, pre):
    """No SH, so campos is unused; the covariance chain under a full rotation still is."""
    cam, cloud, cols, cov = pc.precomp_inputs()
    ref = pc.precomp_reference()
    _lib.tune_set("preprocess", pre)
    hip = hp.run_hip(cloud, cam, 0, _bg(), hip_device, pc.upstream(cam), colors_precomp=cols, cov3D_precomp=cov)
    fwd = hp.compare_forward(hip, ref)
    _report(f"precomp, preprocess {pre}", fwd, hp.compare_grads(hip["grads"], ref["grads"], names=pc.NAMES_PRE))


# ---- b. the raw path ----------------------------------------------------------------------------------------------------------
def _on_device(pc_cpu, dev):
    """The same stored bits on the device, as fresh leaves."""
    out = copy.copy(pc_cpu)
    for n in RAW_PARAMS:
        setattr(out, n, getattr(pc_cpu, n).detach().to(dev).requires_grad_(True))
    return out


def _raw_grads(model):
    return {n: getattr(model, n).grad.detach().cpu().numpy() for n in RAW_PARAMS}


def _forward_of(out):
    return dict(color=out["render"].detach().cpu().numpy(), depth=out["depth"].detach().cpu().numpy(),
                radii=out["radii"].cpu().numpy())


def check_raw_path(hip_device, cases, case):
    """As tests/test_gpu_raw.py: test_raw_matches_cpu_oracle, then test_raw_matches_activated_path at that file's bars.  cases: the
    module of the case (this file's posed_cases; tests/test_gpu_intrinsics.py passes its own)."""
    from luciddreamer_amd.gaussian_renderer import render, render_raw
    cam, pc_cpu, act, degree = cases.raw_cloud(case)
    ref = cases.raw_reference(case)
    camd, bg = cam.to(hip_device), _bg().to(hip_device)
    gcol = cases.upstream(cam, 4).to(hip_device)
    raw = _on_device(pc_cpu, hip_device)
    out_r = render_raw(camd, raw, bg_color=bg)
    (out_r["render"] * gcol).sum().backward()
    hip = _forward_of(out_r)
    assert (hip["radii"] == ref["radii"]).mean() >= 0.999          # the kernels' activations are not bit-identical to torch's
    hp.compare_forward(hip, ref, check_exact=False)
    # the oracle's activated-input gradients chained through the activations in float64
    s, o = act["scales"].double().numpy(), act["opacities"].double().numpy()
    r = pc_cpu._rotation.detach().double().numpy()
    nr = np.linalg.norm(r, axis=1, keepdims=True)
    q = r / nr
    gq = ref["grads"]["rotations"].astype(np.float64)
    want = {"_xyz": ref["grads"]["means3D"], "_scaling": ref["grads"]["scales"] * s,
            "_opacity": ref["grads"]["opacity"].reshape(-1, 1) * o * (1 - o),
            "_rotation": (gq - q * (q * gq).sum(1, keepdims=True)) / nr,
            "_features_dc": ref["grads"]["sh"][:, :1, :], "_features_rest": ref["grads"]["sh"][:, 1:, :]}
    g_r, vs_r = _raw_grads(raw), out_r["viewspace_points"].grad.detach().cpu().numpy()
    for n, e in want.items():
        hp.compare_grads({n: g_r[n]}, {n: e.astype(np.float32)}, names=(n,))
    hp.compare_grads({"vs": vs_r}, {"vs": ref["grads"]["means2D"]}, names=("vs",))
    # ... and the activated path on the same stored tensors
    act_model = _on_device(pc_cpu, hip_device)
    out_a = render(camd, act_model, bg_color=bg)
    (out_a["render"] * gcol).sum().backward()
    g_a, vs_a = _raw_grads(act_model), out_a["viewspace_points"].grad.detach().cpu().numpy()
    assert (out_a["radii"] == out_r["radii"]).float().mean().item() >= 0.999
    cerr = (out_a["render"] - out_r["render"]).abs().max().item()
    derr = (out_a["depth"] - out_r["depth"]).abs().max().item()
    assert cerr <= 2e-5 and derr <= 2e-4, (cerr, derr)
    hp.compare_grads({"vs": vs_r}, {"vs": vs_a}, names=("vs",), rtol=2e-4)
    for n in RAW_PARAMS:
        hp.compare_grads({n: g_r[n]}, {n: g_a[n]}, names=(n,), rtol=2e-4)


@pytest.mark.parametrize("case", pc.RAW_CASES)
def test_raw_path_matches_oracle_and_activated_path(hip_device, case):
    check_raw_path(hip_device, pc, case)


# ---- c. the depth and alpha outputs and their gradients, against the float64 restatement --------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("with_color", [False, True], ids=["depth_only", "color_and_depth"])
@pytest.mark.parametrize("case", pc.MODE_CASES)
def test_depth_loss_matches_float64(hip_device, case, with_color, strict):
    cam, cloud, degree = pc.make(case)
    H, W = cam.image_height, cam.image_width
    gc = pc.upstream(cam) if with_color else torch.zeros(3, H, W)
    config.set_depth_gradient(True)
    config.set_strict_parity(strict)
    fig = dg._check(hip_device, cloud, cam, degree, gc, dg._upstream(H, W, 3))
    print(f"[posed] {case} depth loss: " + ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in fig.items() if s > 0))


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("with_color_depth", [False, True], ids=["alpha_only", "color_depth_alpha"])
@pytest.mark.parametrize("case", pc.MODE_CASES)
def test_alpha_loss_matches_float64(hip_device, case, with_color_depth, strict):
    cam, cloud, degree = pc.make(case)
    config.set_strict_parity(strict)
    fig = al._check(hip_device, cloud, cam, degree, with_color_depth)
    print(f"[posed] {case} alpha loss: " + ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in fig.items() if s > 0))


@pytest.mark.parametrize("case", pc.MODE_CASES)
def test_depth_and_alpha_images_match_float64(hip_device, case):
    cam, cloud, degree = pc.make(case)
    ref = al._oracle(cloud, cam, degree, _bg())
    hip = al._run(cloud, cam, degree, _bg(), hip_device)
    assert np.array_equal(hip["radii"].numpy(), ref["radii"].numpy())
    d_ref = ref["depth"]
    d_err = float(((hip["depth"].double() - d_ref).abs() / d_ref.abs().clamp(min=1.0)).max())
    a_err = float((hip["alpha"].double() - ref["alpha"]).abs().max())
    c_err = float((hip["color"].double() - ref["color"]).abs().max())
    print(f"[posed] {case}: depth image {d_err:.2e} (relative), alpha {a_err:.2e}, colour {c_err:.2e} against float64")
    assert float(d_ref.max()) > 1.0
    assert d_err <= hp.DEPTH_RTOL and a_err <= hp.COLOR_ATOL and c_err <= hp.COLOR_ATOL


# ---- d. anti-aliasing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
def test_antialiased_matches_the_composed_expectation(hip_device, strict):
    """As tests/test_gpu_aa.py::test_gradients_match_the_composed_expectation, under the general pose: aa_ref.coef32 / coef64
    take the view matrix."""
    from tests import aa_cases
    from tests.test_gpu_aa import _compose
    cam, cloud = pc.aa_inputs()
    ref = pc.aa_reference()
    coef = aa_cases.coef_of(cam, cloud)
    exp = _compose(ref["grads"], cam, cloud, coef)
    config.set_strict_parity(strict)
    config.set_antialiasing(True)
    hip = hp.run_hip(cloud, cam, 3, _bg(), hip_device, pc.upstream(cam))
    fwd = hp.compare_forward(hip, ref)
    _report("antialiased", fwd, hp.compare_grads(hip["grads"], exp, names=pc.NAMES_SH))
    for k in ("scales", "rotations"):                     # the coefficient's own derivative is a real share of the expectation
        share = np.abs(exp[k] - ref["grads"][k]).max() / np.abs(exp[k]).max()
        assert share > 10 * hp.GRAD_RTOL, (k, share)
    config.set_antialiasing(False)
    plain = hp.run_hip(cloud, cam, 3, _bg(), hip_device)
    assert np.abs(plain["color"] - hip["color"]).max() > 1e-3


# ---- e. the multi-view step: five different poses in one call -----------------------------------------------------------------
def _raster(cam, bg):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    tfx, tfy = hp.tan_fov(cam)
    return GaussianRasterizer(GaussianRasterizationSettings(cam.image_height, cam.image_width, tfx, tfy, bg, 1.0,
                                                            cam.world_view_transform, cam.full_proj_transform, 3,
                                                            cam.camera_center, False, False))


class _Step:
    """The step's scene on the device in a given order of the views."""

    def __init__(self, dev, order=None, cases=pc):
        cams, cloud = cases.step_scene()
        self.order = list(range(len(cams))) if order is None else list(order)
        self.dev = dev
        self.cams = [cams[i].to(dev) for i in self.order]
        self.gs = [cases.step_upstream(i).to(dev) for i in self.order]
        self.cloud = {k: v.to(dev) for k, v in cloud.items()}
        self.bg = _bg().to(dev)
        self.P, self.W, self.H = cloud["means3D"].shape[0], cams[0].image_width, cams[0].image_height

    def per_view(self, loss_fn, model=None):
        """Every view through the operator, gradients accumulated by autograd; loss_fn(k, colour, depth) is view k's loss (k: the
        position in this order).  model: densify.add_densification_stats after every view.  Returns (gradients in the step's
        naming, depth images, loss values)."""
        leaf = {k: v.clone().requires_grad_(True) for k, v in self.cloud.items()}
        m2d_sum = torch.zeros(self.P, 3, device=self.dev)
        depths, values = [], []
        for k, cam in enumerate(self.cams):
            m2d = torch.zeros(self.P, 3, device=self.dev, requires_grad=True)
            col, radii, dep = _raster(cam, self.bg)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"],
                                                    shs=leaf["shs"], scales=leaf["scales"], rotations=leaf["rotations"])
            loss = loss_fn(k, col, dep)
            loss.backward()
            values.append(float(loss.detach()))
            depths.append(dep.detach().clone())
            m2d_sum += m2d.grad
            if model is not None:
                densify.add_densification_stats(model, m2d, radii)
        grads = {k: leaf[name].grad for k, name in ACC_OF.items() if k != "means2D"}
        grads["means2D"] = m2d_sum
        return grads, depths, values

    def zeros(self):
        shapes = {"means3D": (self.P, 3), "means2D": (self.P, 3), "opacity": (self.P, 1), "sh": (self.P, 16, 3),
                  "scales": (self.P, 3), "rotations": (self.P, 4)}
        return {k: torch.zeros(s, device=self.dev) for k, s in shapes.items()}

    def run(self, batch, stats=None):
        acc = self.zeros()
        c = self.cloud
        with torch.no_grad():
            batch.run(c["means3D"], c["opacities"], c["scales"], c["rotations"], c["shs"], acc, stats=stats)
        batch.check()
        return acc

    def images(self):
        return [torch.zeros(1, self.H, self.W, device=self.dev) for _ in self.cams]


CAPACITY = 200_000


def _close(got, want, what, tol=VIEW_TOL):
    a, b = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    scale = np.abs(b).max()
    assert scale > 0, what
    err = np.abs(a - b).max()
    assert np.isfinite(a).all() and err <= tol * scale, (what, err, scale)
    return err / scale


def _depth_against_oracle(depth, view, what, cases=pc):
    ref = cases.step_reference(view)["depth"]
    err = float((np.abs(depth.cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref))).max())
    assert err <= hp.DEPTH_RTOL, (what, err)
    return err


@pytest.mark.parametrize("n_streams", [1, 2, 3])
def test_step_of_five_poses_matches_oracle_and_per_view_runs(hip_device, n_streams):
    st = _Step(hip_device)
    depths = st.images()
    batch = parallel.ViewBatch(st.cams, st.gs, 3, st.bg, binning_capacity=CAPACITY, n_streams=n_streams, depths=depths)
    acc = st.run(batch)
    # every view's depth image against THAT view's oracle depth: a view matrix taken from another slot shows here
    d = [_depth_against_oracle(depths[k], v, f"view {v}") for k, v in enumerate(st.order)]
    # the sums against the sum of the per-view oracle gradients
    want = {k: sum(pc.step_reference(v)["grads"][k].astype(np.float64) for v in st.order) for k in pc.NAMES_SH}
    fig = hp.compare_grads({k: acc[k].double().cpu().numpy() for k in pc.NAMES_SH}, want, names=pc.NAMES_SH)
    # ... and against per-view autograd accumulation on the device
    hip, hip_depths, _ = st.per_view(lambda k, col, dep: (col * st.gs[k]).sum())
    rel = {k: _close(acc[k], hip[k], k) for k in ACC_OF}
    for k in range(len(st.cams)):
        _close(depths[k], hip_depths[k], f"depth {k}", tol=1e-5)
    print(f"[posed] step, {n_streams} chain(s): depth images {max(d):.2e}; against the oracle sums " +
          ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in fig.items()) + "; against per-view runs " +
          ", ".join(f"{k} {v:.2e}" for k, v in rel.items()))


def test_step_with_targets_matches_per_view_losses(hip_device):
    from luciddreamer_amd.loss import l1_dssim_loss
    st = _Step(hip_device)
    gen = torch.Generator().manual_seed(3)
    targets = [torch.rand(3, st.H, st.W, generator=gen).to(hip_device) for _ in st.cams]
    hip, _, values = st.per_view(lambda k, col, dep: l1_dssim_loss(col, targets[k], 0.2))
    batch = parallel.ViewBatch(st.cams, None, 3, st.bg, binning_capacity=CAPACITY, n_streams=2, targets=targets, lambda_dssim=0.2)
    acc = st.run(batch)
    got = batch.losses.cpu().numpy()[:, 0]
    assert np.abs(got - np.array(values)).max() <= 1e-5 * np.abs(values).max(), (got, values)
    assert len(set(np.round(values, 6))) == len(values)              # five different views, five different losses
    for k in ACC_OF:
        _close(acc[k], hip[k], k)


def test_step_with_depth_targets_matches_per_view_losses(hip_device):
    from luciddreamer_amd.loss import depth_l1, l1_dssim_loss
    from tests.test_gpu_depth_views import _depth_targets
    st = _Step(hip_device)
    w = 0.35
    gen = torch.Generator().manual_seed(4)
    targets = [torch.rand(3, st.H, st.W, generator=gen).to(hip_device) for _ in st.cams]
    dts = _depth_targets(hip_device, st.cams, st.W, st.H, 70)
    config.set_depth_gradient(True)
    pairs = []

    def loss(k, col, dep):
        lc, ld = l1_dssim_loss(col, targets[k], 0.2), depth_l1(dep, dts[k])
        pairs.append((float(lc.detach()) + w * float(ld.detach()), float(ld.detach())))
        return lc + w * ld
    hip, _, _ = st.per_view(loss)
    config.set_depth_gradient(False)
    depths = st.images()
    batch = parallel.ViewBatch(st.cams, None, 3, st.bg, binning_capacity=CAPACITY, n_streams=3, targets=targets, lambda_dssim=0.2,
                               depth_targets=dts, depth_weight=w, depths=depths)
    acc = st.run(batch)
    got, want = batch.losses.cpu().numpy(), np.array(pairs)
    assert np.all(want[:, 1] > 0)
    assert np.abs(got[:, 0] - want[:, 0]).max() <= 1e-5 * np.abs(want[:, 0]).max()
    assert np.abs(got[:, 3] - want[:, 1]).max() <= 1e-5 * np.abs(want[:, 1]).max()
    for k in ACC_OF:
        _close(acc[k], hip[k], k)
    for k, v in enumerate(st.order):
        _depth_against_oracle(depths[k], v, f"view {v}")


def test_step_with_densify_stats_matches_per_view_statistics(hip_device):
    """densify_stats="grad": as if densify.add_densification_stats had run after every view with that view's own screen-space
    gradient and radii.  The norm sum at the bar of tests/test_gpu_views_stats.py (helpers.compare_grads), the rest exact."""
    st = _Step(hip_device)
    P = st.P
    model = SimpleNamespace(xyz_gradient_accum=torch.zeros(P, 1, device=hip_device), denom=torch.zeros(P, 1, device=hip_device),
                            max_radii2D=torch.zeros(P, device=hip_device))
    hip, _, _ = st.per_view(lambda k, col, dep: (col * st.gs[k]).sum(), model=model)
    stats = {"xyz_gradient_accum": torch.zeros(P, 1, device=hip_device), "denom": torch.zeros(P, 1, device=hip_device),
             "max_radii2D": torch.zeros(P, device=hip_device)}
    batch = parallel.ViewBatch(st.cams, st.gs, 3, st.bg, binning_capacity=CAPACITY, n_streams=2, densify_stats="grad")
    acc = st.run(batch, stats)
    assert torch.equal(stats["denom"], model.denom) and torch.equal(stats["max_radii2D"], model.max_radii2D)
    assert float(model.denom.max()) >= 2.0 and float(model.denom.min()) == 0.0      # seen by several poses, and by none
    hp.compare_grads({"accum": stats["xyz_gradient_accum"].double().cpu().numpy()},
                     {"accum": model.xyz_gradient_accum.double().cpu().numpy()}, names=["accum"])
    for k in ACC_OF:
        _close(acc[k], hip[k], k)


def test_step_in_reversed_order_gives_the_same_views(hip_device):
    """The same five views in reversed order: every view's depth image keeps its bits, the sums agree.  The blend shapes are
    pinned, as wherever steps are compared to the bit (the library picks them by the number of views in flight otherwise)."""
    _lib.tune_set("blend_quad", 2)
    _lib.tune_set("fwd_pair", 2)
    results = []
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0]):
        st = _Step(hip_device, order)
        depths = st.images()
        batch = parallel.ViewBatch(st.cams, st.gs, 3, st.bg, binning_capacity=CAPACITY, n_streams=2, depths=depths)
        acc = st.run(batch)
        results.append((acc, {v: depths[k] for k, v in enumerate(order)}))
    (acc_f, dep_f), (acc_r, dep_r) = results
    for v in dep_f:
        assert float(dep_f[v].abs().max()) > 0
        assert torch.equal(dep_f[v], dep_r[v]), v
    for k in ACC_OF:
        _close(acc_r[k], acc_f[k], k)


# ---- f. the layers that unpack a camera object -------------------------------------------------------------------------------
def test_render_and_dropin_with_a_posed_minicam(hip_device):
    from luciddreamer_amd import dropin
    from luciddreamer_amd.gaussian_renderer import render
    case = "box_general"
    cam, pc_cpu, _, _ = pc.raw_cloud(case)
    ref = pc.raw_reference(case)
    camd, bg = cam.to(hip_device), _bg().to(hip_device)
    model = _on_device(pc_cpu, hip_device)
    out = render(camd, model, bg_color=bg)

    def reference_render(*args, **kw):
        raise AssertionError("the reference's render must have been replaced")
    ns = SimpleNamespace(render=reference_render)
    opt = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    h = dropin.install(ns, None, None, losses=False, adam=False, stats=False)
    try:
        dropped = ns.render(camd, model, opt, bg)
    finally:
        dropin.uninstall(h)
    for what, o in (("render", out), ("drop-in", dropped)):
        hip = dict(color=o["render"].detach().cpu().numpy(), depth=o["depth"].detach().cpu().numpy(),
                   radii=torch.as_tensor(o["radii"]).cpu().numpy())
        assert (hip["radii"] == ref["radii"]).mean() >= 0.999, what
        fig = hp.compare_forward(hip, ref, check_exact=False)
        print(f"[posed] {what} with a posed MiniCam: colour {fig['color_max']:.2e}, depth {fig['depth_rel_max']:.2e}")
