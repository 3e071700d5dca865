"""Camera intrinsics on the GPU: wide and narrow fields of view, non-square pixels (focal_x != focal_y), a shifted principal
point and another near / far pair against the references.

Everywhere else in the suite a camera comes from cameras.make_camera: one field of view, FoVy from the aspect ratio, a centred
axis, and in a multi-view step one set of intrinsics for every view -- so tan_fovx, tan_fovy and the third column of the
projection matrix never leave one point in a compared run, although the kernels take them independently.  Here every code path
that takes them runs under the rows of tests/intrinsics_cases.py: the operator with both preprocess kernels, the raw path, the
depth and alpha outputs and their gradients, anti-aliasing, the side outputs, the pooled off-screen test, the multi-view step
with five different intrinsics in one call (with each of its loss options), and the Python consumers of FoVx / FoVy.
tests/test_intrinsics_cases_cpu.py checks on the CPU that every case used here is fit for its comparison (no threshold-fragile
pixel, so gradients are held to the whole-tensor bar) and that each differs by 100 bars or more under the bugs it aims at.
Tolerances are the project's own (tests/helpers.py and the files the comparisons are borrowed from).

The absolute gradient is left out: its float64 reference (tests/absgrad_ref.py) is tied to the identity-camera cases of
tests/absgrad_cases.py.  tsdf.pinhole_of, filter3d and normals.depth_normals document a centred principal point: they are run
under non-square pixels only."""

import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, config, parallel
from tests import helpers as hp, intrinsics_cases as ic
from tests import test_gpu_alpha as al
from tests import test_gpu_depth_grad as dg
from tests import test_gpu_posed as tp
from tests.test_screen_cull_cpu import sc              # noqa: F401 -- the host build of csrc/screen_cull.h, as a fixture

pytestmark = pytest.mark.gpu

PRE_IDS = tp.PRE_IDS
ACC_OF = tp.ACC_OF
CAPACITY = tp.CAPACITY


@pytest.fixture(autouse=True)
def _restore():
    yield
    for knob in ("preprocess", "pcull", "blend_quad", "fwd_pair"):
        _lib.tune_set(knob, -1)
    config.set_depth_gradient(False)
    config.set_strict_parity(False)
    config.set_antialiasing(False)


@pytest.fixture
def exact_mode():
    """Bit comparisons between calls: every forward in exact mode (async mode's binning bound can pick another shape)."""
    config.set_async(False)
    yield
    config.set_async(True)
    config.reset()


def _bg():
    return torch.tensor(ic.BG)


def _report(what, fwd, grads):
    print(f"[intrinsics] {what}: colour {fwd['color_max']:.2e}, depth {fwd['depth_rel_max']:.2e}, gradients " +
          ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in grads.items() if s > 0))


# ---- 1. the operator, forward and backward, against the C oracle --------------------------------------------------------------
@pytest.mark.parametrize("pre", [0, 1], ids=PRE_IDS)
@pytest.mark.parametrize("case", ic.CASES)
def test_operator_matches_oracle(hip_device, case, pre):
    cam, cloud, degree = ic.make(case)
    ref = ic.reference(case)
    _lib.tune_set("preprocess", pre)
    hip = hp.run_hip(cloud, cam, degree, _bg(), hip_device, ic.upstream(cam))
    fwd = hp.compare_forward(hip, ref)
    assert float(np.abs(ref["grads"]["means3D"]).max()) > 0
    _report(f"{case}, preprocess {pre}", fwd, hp.compare_grads(hip["grads"], ref["grads"], names=ic.NAMES_SH))


# ---- 2. the caller's own colours and covariances --------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", [0, 1], ids=PRE_IDS)
def test_operator_with_own_colours_and_covariances(hip_device, pre):
    cam, cloud, cols, cov = ic.precomp_inputs()
    ref = ic.precomp_reference()
    _lib.tune_set("preprocess", pre)
    hip = hp.run_hip(cloud, cam, 0, _bg(), hip_device, ic.upstream(cam), colors_precomp=cols, cov3D_precomp=cov)
    fwd = hp.compare_forward(hip, ref)
    _report(f"precomp, preprocess {pre}", fwd, hp.compare_grads(hip["grads"], ref["grads"], names=ic.NAMES_PRE))


# ---- 3. the raw path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ic.RAW_CASES)
def test_raw_path_matches_oracle_and_activated_path(hip_device, case):
    tp.check_raw_path(hip_device, ic, case)


# ---- 4. the depth and alpha outputs and their gradients, against the float64 restatement --------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("with_color", [False, True], ids=["depth_only", "color_and_depth"])
@pytest.mark.parametrize("case", ic.MODE_CASES)
def test_depth_loss_matches_float64(hip_device, case, with_color, strict):
    cam, cloud, degree = ic.make(case)
    H, W = cam.image_height, cam.image_width
    gc = ic.upstream(cam) if with_color else torch.zeros(3, H, W)
    config.set_depth_gradient(True)
    config.set_strict_parity(strict)
    fig = dg._check(hip_device, cloud, cam, degree, gc, dg._upstream(H, W, 3))
    print(f"[intrinsics] {case} depth loss: " + ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in fig.items() if s > 0))


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("with_color_depth", [False, True], ids=["alpha_only", "color_depth_alpha"])
@pytest.mark.parametrize("case", ic.MODE_CASES)
def test_alpha_loss_matches_float64(hip_device, case, with_color_depth, strict):
    cam, cloud, degree = ic.make(case)
    config.set_strict_parity(strict)
    fig = al._check(hip_device, cloud, cam, degree, with_color_depth)
    print(f"[intrinsics] {case} alpha loss: " + ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in fig.items() if s > 0))


@pytest.mark.parametrize("case", ic.MODE_CASES)
def test_depth_and_alpha_images_match_float64(hip_device, case):
    cam, cloud, degree = ic.make(case)
    ref = al._oracle(cloud, cam, degree, _bg())
    hip = al._run(cloud, cam, degree, _bg(), hip_device)
    assert np.array_equal(hip["radii"].numpy(), ref["radii"].numpy())
    d_ref = ref["depth"]
    d_err = float(((hip["depth"].double() - d_ref).abs() / d_ref.abs().clamp(min=1.0)).max())
    a_err = float((hip["alpha"].double() - ref["alpha"]).abs().max())
    c_err = float((hip["color"].double() - ref["color"]).abs().max())
    print(f"[intrinsics] {case}: depth image {d_err:.2e} (relative), alpha {a_err:.2e}, colour {c_err:.2e} against float64")
    assert float(d_ref.max()) > 1.0
    assert d_err <= hp.DEPTH_RTOL and a_err <= hp.COLOR_ATOL and c_err <= hp.COLOR_ATOL


# ---- 5. anti-aliasing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
def test_antialiased_matches_the_composed_expectation(hip_device, strict):
    """As tests/test_gpu_aa.py::test_gradients_match_the_composed_expectation: aa_ref.coef32 / coef64 take the tangents."""
    from tests import aa_cases
    from tests.test_gpu_aa import _compose
    cam, cloud = ic.aa_inputs()
    ref = ic.aa_reference()
    coef = aa_cases.coef_of(cam, cloud)
    exp = _compose(ref["grads"], cam, cloud, coef)
    config.set_strict_parity(strict)
    config.set_antialiasing(True)
    hip = hp.run_hip(cloud, cam, 3, _bg(), hip_device, ic.upstream(cam))
    fwd = hp.compare_forward(hip, ref)
    _report("antialiased", fwd, hp.compare_grads(hip["grads"], exp, names=ic.NAMES_SH))
    for k in ("scales", "rotations"):                     # the coefficient's own derivative is a real share of the expectation
        share = np.abs(exp[k] - ref["grads"][k]).max() / np.abs(exp[k]).max()
        assert share > 10 * hp.GRAD_RTOL, (k, share)
    config.set_antialiasing(False)
    plain = hp.run_hip(cloud, cam, 3, _bg(), hip_device)
    assert np.abs(plain["color"] - hip["color"]).max() > 1e-3


# ---- 6. the side outputs, each at the bar of its own suite --------------------------------------------------------------------
REF_KEY = dict(means3D="means3D", means2D="means2D", opacities="opacity", shs="sh", scales="scales", rotations="rotations",
               features="features")
GEO = ["means3D", "means2D", "opacity", "scales", "rotations"]
FWD_BAR = 4.0               # x the float32 walk's distance from float64 (render_normals_ref.FWD_ERR's margin)


def _side_grads(what, got, leaf, names):
    got = {REF_KEY[k]: v for k, v in got.items()}
    fig = hp.compare_grads(got, leaf, names=names)
    print(f"[intrinsics] {what} gradients: " + ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in fig.items()))


def test_median_depth_matches_the_reference_walk(hip_device, exact_mode):
    """As tests/test_gpu_median.py::test_parity_with_the_reference_walk."""
    from tests import median_ref as mr
    from tests.test_gpu_median import _run
    cam, cloud, degree = ic.make(ic.SIDE_CASE)
    r = ic.median_reference()
    n_pix = r["ids"].size
    assert r["fragile"].sum() <= mr.FRAGILE_CAP * n_pix
    o = _run(cloud, cam, degree, _bg(), hip_device)
    ids, depth = o["median_ids"], o["median_depth"][0]
    differ = ids != r["ids"]
    print(f"[intrinsics] median: {int(differ.sum())} pixels differ, {int(r['fragile'].sum())} fragile")
    assert not (differ & ~r["fragile"]).any()
    assert differ.sum() <= mr.FRAGILE_CAP * n_pix
    has = ids >= 0
    want = r["st"]["depths"][ids[has]]
    assert has.mean() > 0.5
    assert (np.abs(depth[has] - want) <= hp.DEPTH_RTOL * np.maximum(1.0, np.abs(want))).all()
    assert not depth[~has].any() and (ids[~has] == -1).all()


def test_rendered_normals_match_float64(hip_device, exact_mode):
    """As tests/test_gpu_render_normals.py: the forward within 4 x the float32 walk's own error, every leaf at GRAD_RTOL."""
    from tests import render_normals_ref as rn
    from tests.test_gpu_render_normals import _run
    cam, cloud, degree = ic.make(ic.SIDE_CASE)
    r = ic.normals_reference()
    ok = ~r["fragile"]
    assert r["fragile"].sum() <= rn.FRAGILE_CAP * r["fragile"].size
    assert np.abs(r["margin"][r["visible"]]).min() > rn.FLIP_BAND
    act = _run(cloud, cam, degree, _bg(), hip_device, gn=r["G"])
    err = float(np.abs(act["normals"].astype(np.float64) - r["N64"])[:, ok].max())
    print(f"[intrinsics] normals: err {err:.3e}, bar {FWD_BAR * r['fwd_err']:.3e}")
    assert err <= FWD_BAR * r["fwd_err"]
    assert not act["normals"][:, ok & (r["layers64"] == 0)].any() and act["normals"][:, ok & (r["layers64"] > 0)].any()
    _side_grads("normals", act["grads"], r["leaf"], GEO)
    assert not act["grads"]["shs"].any()


def test_distortion_matches_float64(hip_device, exact_mode):
    """As tests/test_gpu_distort.py, linear mapping."""
    from tests import distort_ref as dr
    from tests.test_gpu_distort import _run
    cam, cloud, degree = ic.make(ic.SIDE_CASE)
    r = ic.distortion_reference()
    ok = ~r["fragile"]
    assert r["fragile"].sum() <= dr.FRAGILE_CAP * r["fragile"].size
    act = _run(cloud, cam, degree, _bg(), hip_device, ic.SIDE_MAPPING, gd=r["G"])
    D = act["distortion"][0]
    err = float(np.abs(D.astype(np.float64) - r["D64"])[ok].max())
    print(f"[intrinsics] distortion: err {err:.3e}, bar {FWD_BAR * r['fwd_err']:.3e}, D max {r['D64'].max():.3e}")
    assert err <= FWD_BAR * r["fwd_err"]
    assert (D >= 0).all() and not D[ok & (r["layers64"] < 2)].any() and D[ok & (r["layers64"] >= 2)].any()
    _side_grads("distortion", act["grads"], r["leaf"], GEO)
    assert not act["grads"]["shs"].any()


def test_feature_map_matches_float64(hip_device, exact_mode):
    """As tests/test_gpu_features.py, a full chunk and a tail."""
    from tests import feature_ref as fr
    from tests.test_gpu_features import _run
    cam, cloud, degree = ic.make(ic.SIDE_CASE)
    r = ic.features_reference()
    ok = ~r["fragile"]
    assert r["fragile"].sum() <= fr.FRAGILE_CAP * r["fragile"].size
    act = _run(cloud, cam, degree, _bg(), hip_device, feats=r["feats"], gf=r["G"])
    F = act["features"]
    err = float(np.abs(F.astype(np.float64) - r["F64"])[:, ok].max())
    print(f"[intrinsics] features: err {err:.3e}, bar {FWD_BAR * r['fwd_err']:.3e}")
    assert F.shape[0] == ic.SIDE_CHANNELS and err <= FWD_BAR * r["fwd_err"]
    assert not F[:, ok & (r["layers32"] == 0)].any() and F[:, ok & (r["layers32"] > 0)].any()
    _side_grads("features", act["grads"], r["leaf"], GEO + ["features"])
    assert not act["grads"]["shs"].any()
    assert np.array_equal(act["radii"] > 0, r["visible"]) and (~r["visible"]).any()
    assert not act["grads"]["features"][~r["visible"]].any()


# ---- 7. the pooled preprocess kernel's off-screen test --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ic.CULL_CASES)
def test_pooled_off_screen_test_leaves_every_bit(hip_device, sc, case):              # noqa: F811
    """tests/test_gpu_screen_cull.py's comparison: header, radii, records, ranges, emission order and both images keep their bits
    with the test on and off, and against the thread-per-Gaussian kernel.  That the test does reject rows of the case is read
    from the host build of the same header, which is what decides on the device too."""
    from tests.test_gpu_screen_cull import _on_off
    cam, cloud, _ = ic.make(case)
    near, rej = sc(cloud, cam)
    u = _on_off(cloud, cam, hip_device)
    print(f"[intrinsics] {case}: off-screen test rejects {int((near & rej).sum())} rows, {int((u['radii'] > 0).sum())} visible")
    assert (near & rej).sum() >= 1
    assert np.array_equal(u["radii"], ic.reference(case)["radii"])
    assert not (u["radii"][near & rej] != 0).any()


# ---- 8. the multi-view step: five poses and five intrinsics in one call ------------------------------------------------------
def _depths_against_oracle(depths, order):
    return max(tp._depth_against_oracle(depths[k], v, f"view {v}", cases=ic) for k, v in enumerate(order))


@pytest.mark.parametrize("n_streams", [1, 2, 3])
def test_step_of_five_intrinsics_matches_oracle_and_per_view_runs(hip_device, n_streams):
    st = tp._Step(hip_device, cases=ic)
    depths = st.images()
    batch = parallel.ViewBatch(st.cams, st.gs, 3, st.bg, binning_capacity=CAPACITY, n_streams=n_streams, depths=depths)
    acc = st.run(batch)
    # every view's depth image against THAT view's oracle depth
    d = _depths_against_oracle(depths, st.order)
    # the sums against the sum of the per-view oracle gradients: tangents taken from another slot show here
    want = {k: sum(ic.step_reference(v)["grads"][k].astype(np.float64) for v in st.order) for k in ic.NAMES_SH}
    fig = hp.compare_grads({k: acc[k].double().cpu().numpy() for k in ic.NAMES_SH}, want, names=ic.NAMES_SH)
    # ... and against per-view autograd accumulation on the device
    hip, hip_depths, _ = st.per_view(lambda k, col, dep: (col * st.gs[k]).sum())
    rel = {k: tp._close(acc[k], hip[k], k) for k in ACC_OF}
    for k in range(len(st.cams)):
        tp._close(depths[k], hip_depths[k], f"depth {k}", tol=1e-5)
    print(f"[intrinsics] step, {n_streams} chain(s): depth images {d:.2e}; against the oracle sums " +
          ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in fig.items()) + "; against per-view runs " +
          ", ".join(f"{k} {v:.2e}" for k, v in rel.items()))


def _render_alpha(cam, bg, leaf, m2d):
    return tp._raster(cam, bg)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"], shs=leaf["shs"],
                               scales=leaf["scales"], rotations=leaf["rotations"], return_alpha=True)


def test_step_with_the_fused_loss_matches_per_view_losses(hip_device):
    """Targets, depth targets and masks in one call against the per-view recipe of tests/test_gpu_mask_views.py (masked L1 + DSSIM,
    the alpha hole term, the depth L1), one operator call and one autograd backward per view, at that file's bars."""
    from luciddreamer_amd.loss import depth_l1, masked_l1_dssim
    from tests import mask_loss_ref
    from tests.test_gpu_mask_views import _depth_targets, _holey_targets
    st = tp._Step(hip_device, cases=ic)
    wa, wd = 0.6, 0.35
    targets, masks = _holey_targets(hip_device, st.cams, st.W, st.H, 3)
    dts = _depth_targets(hip_device, st.cams, st.W, st.H, 70)
    config.set_depth_gradient(True)
    leaf = {k: v.clone().requires_grad_(True) for k, v in st.cloud.items()}
    m2d = torch.zeros(st.P, 3, device=hip_device, requires_grad=True)
    rows = []
    for i, cam in enumerate(st.cams):
        col, _, dep, alp = _render_alpha(cam, st.bg, leaf, m2d)
        lc = masked_l1_dssim(col, targets[i], masks[i], 0.2)
        la = mask_loss_ref.torch_alpha_hole(alp, masks[i])
        ld = depth_l1(dep, dts[i])
        loss = lc + wa * la + wd * ld
        loss.backward()
        rows.append([float(loss.detach()), float(ld.detach()), float(la.detach())])
    config.set_depth_gradient(False)
    want = {k: leaf[name].grad for k, name in ACC_OF.items() if k != "means2D"}
    want["means2D"] = m2d.grad
    depths, alphas = st.images(), st.images()
    batch = parallel.ViewBatch(st.cams, None, 3, st.bg, binning_capacity=CAPACITY, n_streams=3, targets=targets, lambda_dssim=0.2,
                               masks=masks, alpha_weight=wa, depth_targets=dts, depth_weight=wd, depths=depths, alphas=alphas)
    acc = st.run(batch)
    got, rows = batch.losses.cpu().numpy(), np.array(rows)
    assert got.shape == (len(st.cams), 5)
    for j, r in ((0, 0), (3, 1), (4, 2)):
        assert np.all(rows[:, r] > 0)
        assert np.abs(got[:, j] - rows[:, r]).max() <= 1e-5 * np.abs(rows[:, r]).max(), (j, got[:, j], rows[:, r])
    assert len(set(np.round(rows[:, 0], 6))) == len(rows)               # five different views, five different losses
    rel = {k: tp._close(acc[k], want[k], k) for k in ACC_OF}
    print("[intrinsics] step with the fused loss against per-view losses: " + ", ".join(f"{k} {v:.2e}" for k, v in rel.items()))
    _depths_against_oracle(depths, st.order)
    with torch.no_grad():
        for cam, a in zip(st.cams, alphas):
            tp._close(a, _render_alpha(cam, st.bg, st.cloud, torch.zeros(st.P, 3, device=hip_device))[3], "alpha", tol=1e-5)


def test_step_with_the_geometry_terms_matches_the_per_view_route(hip_device):
    """Distortion and normal consistency in the step against tests/test_gpu_geom_views.py's per-view route, at its bars: the only
    comparison that can tell the tangents the normal term of view v is handed from view 0's."""
    from tests import test_gpu_geom_views as gv
    st = tp._Step(hip_device, cases=ic)
    gen = torch.Generator().manual_seed(11)
    targets = [torch.rand(3, st.H, st.W, generator=gen).to(hip_device) for _ in st.cams]
    config.set_depth_gradient(True)           # the per-view route differentiates the depth output (the fixture switches it off)
    ref, rows, maps, c64 = gv._per_view(st.cloud, st.cams, targets, st.bg, gv.W_D, gv.W_N)
    config.set_depth_gradient(False)
    acc, losses, _ = gv._step(st.cloud, st.cams, targets, st.bg, 2, distortion_weight=gv.W_D, distortion_map=gv.MAPPING,
                              normal_consistency_weight=gv.W_N)
    gv._compare_acc(acc, ref, "[intrinsics] geometry step")
    # the band cloud is thin in these views: 15 to 35 % of the pixels have a depth, 3.6 to 20 % a normal from depth (a pixel and
    # its four neighbours) -- some hundreds of terms in the least covered view
    gv._compare_losses(losses, rows, maps, c64, gv.W_D, gv.W_N, "[intrinsics] geometry step", min_valid=0.03)
    plain, _, _ = gv._step(st.cloud, st.cams, targets, st.bg, 2)
    for k in ("means3D", "scales", "rotations"):
        assert float((plain[k] - acc[k]).abs().max()) > 100 * hp.GRAD_RTOL * float(acc[k].abs().max()), k


# ---- 9. near and far ------------------------------------------------------------------------------------------------------------
def test_znear_and_zfar_do_not_reach_the_outputs(hip_device, exact_mode):
    """The kernels never read the third clip row: (0.5, 20) and (0.01, 100) give the same bits."""
    cam, cloud, degree = ic.make("general")
    other = ic.row_camera("general", znear=0.01, zfar=100.0)
    assert (cam.znear, cam.zfar) == (0.5, 20.0) and not torch.equal(other.full_proj_transform, cam.full_proj_transform)
    for pre in (0, 1):
        _lib.tune_set("preprocess", pre)
        a = hp.run_hip(cloud, cam, degree, _bg(), hip_device, ic.upstream(cam))
        b = hp.run_hip(cloud, other, degree, _bg(), hip_device, ic.upstream(cam))
        for k in ("color", "depth", "radii"):
            assert np.array_equal(a[k], b[k]), (pre, k)
        assert a["color"].any() and (a["radii"] > 0).any()
        for k in ic.NAMES_SH:
            assert np.array_equal(a["grads"][k], b["grads"][k]), (pre, k)
            assert a["grads"][k].any(), k


# ---- 10. the Python consumers of FoVx / FoVy under non-square pixels ----------------------------------------------------------
@pytest.mark.parametrize("mode", ["median", "expected"])
def test_fuse_views_with_non_square_pixels(hip_device, mode):
    """tests/test_gpu_tsdf.py::test_fuse_views_equals_rendering_and_integrating_by_hand, its wall and its assertions, under three
    cameras with the tangents of "tall_pixels"."""
    from luciddreamer_amd import tsdf
    from luciddreamer_amd.gaussian_renderer import DEFAULT_OPT, render
    from tests.test_gpu_tsdf import FUSE_POSES, _same_bits, _wall
    model = _wall(hip_device)
    bg = torch.tensor([0.1, 0.2, 0.3], device=hip_device)
    tx, ty = ic.tangents("tall_pixels")
    views = [ic.camera(p, 64, 64, tx, ty).to(hip_device) for p in FUSE_POSES]
    make = lambda: tsdf.TSDFVolume((-1.0, -1.0, 2.45), 0.1, (21, 20, 11), 0.3, hip_device)
    fused = tsdf.fuse_views(make(), views, model, DEFAULT_OPT, bg, depth=mode, alpha_min=0.5)
    hand = make()
    with torch.no_grad():
        for view in views:
            out = render(view, model, DEFAULT_OPT, bg, return_alpha=True, return_median=mode == "median")
            alpha = out["alpha"].reshape(64, 64)
            d = out["median_depth"].reshape(64, 64) if mode == "median" else out["depth"].reshape(64, 64) / alpha
            d = torch.where(alpha < 0.5, torch.zeros_like(d), d)
            K = tsdf.pinhole_of(view)[0]
            assert abs(K[0, 0] - 32.0 / tx) <= 1e-9 * K[0, 0] and abs(K[1, 1] - 32.0 / ty) <= 1e-9 * K[1, 1]
            hand.integrate(d, *tsdf.pinhole_of(view), color=out["render"].permute(1, 2, 0).contiguous())
    w = fused.weight.cpu().numpy()
    D = fused.tsdf.cpu().numpy()
    assert (w == 3).any() and (w == 0).any() and (D[w > 0] < 0).any() and (D[w > 0] > 0).any()
    for name in ("tsdf", "weight", "color"):
        _same_bits(name, getattr(fused, name), getattr(hand, name).cpu().numpy())
    V, C, F = fused.extract_mesh(1.0)
    assert F.shape[0] > 0 and float((V[:, 2] - 3.0).abs().max()) < 0.1


def test_filter3d_camera_rows_with_non_square_pixels(hip_device):
    """filter3d.compute_filter_3d on camera OBJECTS with the tangents of "tall_pixels" against tests/filter3d_ref.update on rows
    written out here from the table's tangents, at the bar of tests/test_gpu_filter3d.py::test_update_against_the_reference."""
    from luciddreamer_amd import filter3d
    from tests import filter3d_cases as C, filter3d_ref as R
    from tests.test_gpu_filter3d import bits
    W, H = ic.INTRINSICS["tall_pixels"][:2]
    tx, ty = ic.tangents("tall_pixels")
    cams = [ic.camera(p, W, H, tx, ty) for p in ("rolled", "llff", (0.3, -0.2, 0.0, (0.2, 0.1, -0.4)))]
    rows = np.zeros((len(cams), 20), np.float32)
    for n, c in enumerate(cams):
        rows[n, :16] = c.world_view_transform.numpy().reshape(16)
        rows[n, 16:] = W / (2.0 * tx), H / (2.0 * ty), W, H
    assert rows[0, 16] > 2.5 * rows[0, 17]
    rng = np.random.default_rng(7)
    xyz = C.draw(rng, 1037)
    for _ in range(100):
        bad = R.update(xyz, rows, return_fragile=True)[2].any(axis=1)
        if not bad.any():
            break
        xyz[bad] = C.draw(rng, int(bad.sum()))
    assert not bad.any()
    f64, seen64 = R.update(xyz, rows)
    f32, _ = R.update(xyz, rows, dtype=np.float32)
    e32 = float(np.abs(f32.astype(np.float64) - f64).max())
    f, seen = filter3d.compute_filter_3d(torch.from_numpy(xyz).to(hip_device), [c.to(hip_device) for c in cams], return_seen=True)
    got, seen = f.cpu().numpy()[:, 0], seen.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - f64).max())
    # what a kernel that takes fy for fx (or the square-pixel fy) would see and give
    swapped = rows.copy()
    swapped[:, 16], swapped[:, 17] = rows[:, 17], rows[:, 16]
    fsw, seen_sw = R.update(xyz, swapped)
    print(f"[intrinsics] filter3d: float32 restatement {e32:.3e}, bar {4 * e32:.3e}, device {err:.3e}, seen {int(seen.sum())} of "
          f"{len(seen)}; with fx and fy exchanged: {int((seen_sw != seen64).sum())} rows seen differently, filter off by "
          f"{float(np.abs(fsw - f64).max()):.3e}")
    assert 100 < seen64.sum() < len(seen64) - 100 and (seen_sw != seen64).sum() > 20
    assert np.array_equal(seen, seen64)
    assert err <= 4 * e32, (err, e32)
    assert np.array_equal(bits(got), bits(f32))


def test_depth_normals_of_a_plane_with_non_square_pixels(hip_device):
    """normals.depth_normals on a camera OBJECT with the tangents of "wide_pixels": a tilted plane's analytic depth against
    tests/normal_ref.py in float64, at the bar of tests/test_gpu_normals.py::test_normals_match_the_float64_reference."""
    from luciddreamer_amd import normals
    from tests import normal_ref as nr, rowbar
    from tests.test_gpu_normals import FLOOR
    cam = ic.row_camera("wide_pixels")
    W, H = cam.image_width, cam.image_height
    tx, ty = ic.tangents("wide_pixels")
    n = np.array([0.25, -0.35, 1.0])
    n /= np.linalg.norm(n)
    u = (np.arange(W) + 0.5) * (2.0 * tx / W) - tx
    v = (np.arange(H) + 0.5) * (2.0 * ty / H) - ty
    depth = (4.0 / (n[0] * u[None, :] + n[1] * v[:, None] + n[2])).astype(np.float32)
    assert depth.min() > 1.0
    n64, valid = nr.torch_normals(torch.from_numpy(depth.astype(np.float64)), tx, ty)
    n64, valid = n64.numpy(), valid.numpy()
    n32, v32 = nr.closed_normals(depth, tx, ty, np.float32)
    assert valid[1:-1, 1:-1].all() and np.array_equal(valid, v32)
    # the reference sees the plane: its normal, towards the camera, everywhere inside (float32 depths: 1e-4)
    assert np.abs(n64[:, valid] + n[:, None]).max() <= 1e-4
    e32 = np.abs(n32 - n64).max()
    got = normals.depth_normals(torch.from_numpy(depth).to(hip_device), cam).cpu().numpy()
    err = np.abs(got - n64).max()
    sq = nr.torch_normals(torch.from_numpy(depth.astype(np.float64)), tx, tx * H / W)[0].numpy()
    print(f"[intrinsics] depth_normals: max|n - n64| {err:.3e}, float32 restatement within {e32:.3e}; with square pixels the "
          f"normal would be off by {np.abs(sq - n64).max():.3e}")
    assert np.abs(sq - n64).max() > 0.1
    assert err <= max(rowbar.E32_MARGIN * e32, FLOOR)
    assert not got[:, ~valid].any() and np.array_equal((got != 0).any(axis=0), valid)
