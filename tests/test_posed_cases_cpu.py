"""The conditions of the posed-camera GPU tests (tests/test_gpu_posed.py), checked where there is no GPU, on the very cases of
tests/posed_cases.py: the CPU oracle flags few enough pixels (none where gradients are held to the whole-tensor bar), no case is
trivial, the two CPU references agree under every pose, every case differs by at least 100 times the GPU test's bar when the
camera is altered on the reference side the way a wrong kernel would alter it, and the restatement still equals the compiled
reference bit for bit."""
import numpy as np
import pytest
import torch

from oracle import oracle, ref
from tests import grad_oracle, helpers as hp, posed_cases as pc

CASES = list(pc.OP_CASES)


def _flag_counts(res):
    fr = res["res"].stage()["fragile"]
    return int((fr != 0).sum()), int(((fr & 1) != 0).sum()), int(((fr & 2) != 0).sum())


def _every_reference():
    """(label, helpers.run_oracle result, image pixels) of every oracle run the GPU tests compare with."""
    for case in CASES:
        cam = pc.make(case)[0]
        yield case, pc.reference(case), cam.image_width * cam.image_height
    cam = pc.precomp_inputs()[0]
    yield "precomp " + pc.PRECOMP_CASE, pc.precomp_reference(), cam.image_width * cam.image_height
    for case in pc.RAW_CASES:
        cam = pc.make(case)[0]
        yield "raw " + case, pc.raw_reference(case), cam.image_width * cam.image_height
    cam, _ = pc.aa_inputs()
    yield "antialiased " + pc.AA_CASE, pc.aa_reference(), cam.image_width * cam.image_height
    cams, _ = pc.step_scene()
    for i, name in enumerate(pc.STEP_POSES):
        yield f"step view {i} ({name})", pc.step_reference(i), cams[i].image_width * cams[i].image_height


def test_flagged_pixels_stay_within_the_caps():
    """helpers.compare_forward caps the colour-flagged pixels at max(8, FRAGILE_FRAC pixels); every gradient comparison of the
    GPU tests is helpers.compare_grads (the whole tensor), so no reference may hold a flagged pixel of either kind."""
    for label, res, pixels in _every_reference():
        any_, colour, depth = _flag_counts(res)
        print(f"[posed] {label}: flagged pixels {any_} (colour {colour}, depth {depth}) of {pixels}, "
              f"{int((res['radii'] > 0).sum())} visible of {res['radii'].size}")
        assert colour <= max(8, hp.FRAGILE_FRAC * pixels), label
        assert any_ == 0, label


@pytest.mark.parametrize("case", CASES)
def test_case_is_not_trivial(case):
    scene = pc.OP_CASES[case][0]
    yaw, pitch, roll, t = pc.pose_of(case)
    cam, cloud, _ = pc.make(case)
    V = cam.world_view_transform.numpy().reshape(-1)            # V[k] as the kernels index it
    Pm = cam.full_proj_transform.numpy().reshape(-1)
    if any(t):
        assert np.abs(cam.camera_center.numpy()).max() > 0.09
        assert np.abs(V[12:15]).max() > 0.09 and np.abs(Pm[12:16]).max() > 0.09
    else:
        assert not cam.camera_center.numpy().any() and not V[12:15].any()
    if pitch:
        assert abs(V[6]) > 0.01 and abs(V[9]) > 0.01
    if roll:
        assert abs(V[1]) > 0.1 and abs(V[4]) > 0.1
    res = pc.reference(case)
    visible = int((res["radii"] > 0).sum())
    P = res["radii"].size
    if scene == "box":
        assert visible >= 0.4 * P, (visible, P)
    else:
        p_view = cloud["means3D"].double() @ cam.world_view_transform.double()[:3, :3] + cam.world_view_transform.double()[3, :3]
        behind = int((p_view[:, 2] <= 0.2).sum())
        print(f"[posed] {case}: {visible} visible, {behind} behind the near plane")
        assert visible >= 100 and behind >= 1000, (visible, behind)


def test_poses_isolate_what_the_table_says():
    V = lambda name: pc.camera(name, 97, 61).world_view_transform.numpy().reshape(-1)
    assert V("pitched")[6] != 0 and V("general")[6] != 0
    assert np.array_equal(V("translated")[[0, 1, 2, 4, 5, 6, 8, 9, 10]], np.eye(3, dtype=np.float32).reshape(-1))
    assert V("rolled")[6] == 0 and V("rolled")[2] == 0 and V("rolled")[1] != 0
    assert len(set(pc.STEP_POSES)) == 5 and list(pc.STEP_POSES) != sorted(pc.STEP_POSES)
    centers = [tuple(c.camera_center.tolist()) for c in pc.step_scene()[0]]
    assert len(set(centers)) >= 4                               # (pitched sits at the origin, the other four elsewhere)


def _float64(cam, cloud, degree, gc):
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    p = dict(means3D=leaf(cloud["means3D"]), opacity=leaf(cloud["opacities"]), scales=leaf(cloud["scales"]),
             rotations=leaf(cloud["rotations"]), sh=leaf(cloud["shs"]))
    p["means2D"] = torch.zeros_like(p["means3D"], requires_grad=True)
    tfx, tfy = hp.tan_fov(cam)
    col, dep, radii = grad_oracle.render(p["means3D"], p["opacity"], cam.world_view_transform, cam.full_proj_transform,
                                         cam.camera_center, tfx, tfy, cam.image_height, cam.image_width, torch.tensor(pc.BG),
                                         scales=p["scales"], rotations=p["rotations"], shs=p["sh"], degree=degree,
                                         means2D=p["means2D"], detach_depth=True)
    (col * gc.double()).sum().backward()
    return col.detach().numpy(), dep.detach().numpy(), radii.numpy(), {k: v.grad.numpy() for k, v in p.items()}


@pytest.mark.parametrize("case", CASES)
def test_c_oracle_and_float64_restatement_agree_under_the_pose(case):
    """The C oracle (a float32 forward and backward with float64 sums, as the reference computes) against
    tests/grad_oracle.render in float64 with the depth detached.  Colour and depth: 1e-5, the bar of
    tests/test_depth_grad_cpu.py (and the GPU tests' own).  Gradients: the float32 side's rounding is not a float64 finite
    difference's, so they are held to what this project allows a float32 backward against a reference, helpers.GRAD_RTOL of each
    tensor's maximum -- the GPU tests hold the kernels to either reference at that bar, so the two must agree within it."""
    cam, cloud, degree = pc.make(case)
    res = pc.reference(case)
    col, dep, radii, grads = _float64(cam, cloud, degree, pc.upstream(cam))
    assert np.array_equal(radii, res["radii"])
    c_err = float(np.abs(res["color"] - col).max())
    d_err = float((np.abs(res["depth"] - dep) / np.maximum(1.0, np.abs(dep))).max())
    figures = {}
    for k in pc.NAMES_SH:
        b = grads[k]
        figures[k] = (float(np.abs(res["grads"][k].reshape(b.shape) - b).max()), float(np.abs(b).max()))
    print(f"[posed] {case}: C oracle vs float64: colour {c_err:.2e}, depth (relative) {d_err:.2e}, gradients (of each maximum) " +
          ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in figures.items()))
    assert c_err <= 1e-5 and d_err <= 1e-5
    for k, (e, s) in figures.items():
        assert s > 0, k
        assert e <= hp.GRAD_RTOL * s, (k, e, s)


# ---- sensitivity: the GPU tests would fail on a kernel that is wrong in one of these ways --------------------------------------
def _differences(case, how):
    """The oracle re-run with the camera altered on the reference side, against the reference the GPU test uses: each difference
    as a multiple of the bar the GPU test applies to that quantity."""
    cam, cloud, degree = pc.make(case)
    res = pc.reference(case)
    alt = hp.run_oracle(cloud, pc.altered(cam, how), degree, torch.tensor(pc.BG), pc.upstream(cam))
    out = {"colour": float(np.abs(alt["color"] - res["color"]).max()) / hp.COLOR_ATOL,
           "depth": float((np.abs(alt["depth"] - res["depth"]) / np.maximum(1.0, np.abs(res["depth"]))).max()) / hp.DEPTH_RTOL}
    for k in ("means3D", "sh"):
        scale = float(np.abs(res["grads"][k]).max())
        out[k] = float(np.abs(alt["grads"][k] - res["grads"][k]).max()) / (hp.GRAD_RTOL * scale)
    return out


# what each alteration must move: campos enters the colour through the SH view direction and the gradients of the means and of
# the SH coefficients; the view translation enters the depth output; the 3 x 3 block enters the covariance chain (colour) --
# and the depth wherever V[2] or V[6] is not zero, which a pure roll leaves zero
MUST_MOVE = {"campos": ("colour", "means3D", "sh"), "translation": ("depth",), "transposed": ("colour",)}


@pytest.mark.parametrize("case", CASES)
def test_case_is_sensitive_to_the_camera_bugs_it_aims_at(case):
    aims = pc.aims(case)
    assert aims, case
    for how in aims:
        ratios = _differences(case, how)
        must = list(MUST_MOVE[how])
        yaw, pitch, _, _ = pc.pose_of(case)
        if how == "transposed" and (yaw or pitch):
            must.append("depth")
        print(f"[posed] {case}, {how} altered: difference / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) +
              f"; asserted >= 100: {must}")
        for k in must:
            assert ratios[k] >= 100.0, (case, how, k, ratios[k])


def test_every_alteration_is_aimed_at_by_box_and_band_cases():
    for how in MUST_MOVE:
        hit = [c for c in CASES if how in pc.aims(c)]
        assert any(c.startswith("box") for c in hit) and any(c.startswith("band") for c in hit), how
    for case in ("box_translated", "box_general", "box_llff", "box_back"):
        assert {"campos", "translation"} <= set(pc.aims(case)), case
    for case in ("box_pitched", "box_rolled", "box_general"):
        assert "transposed" in pc.aims(case), case


def test_step_views_differ_from_each_other_by_far_more_than_the_bar():
    """A step that handed every view the first view's campos (or view matrix) would have to fail: every view's reference, re-run
    with view 0's campos, differs from its own by 100 bars in colour -- wherever the two positions differ -- and every pair of
    views' depth images differs by 100 bars."""
    cams, cloud = pc.step_scene()
    first = cams[0]
    for i in range(1, len(cams)):
        res = pc.step_reference(i)
        alt = hp.run_oracle(cloud, cams[i]._replace(camera_center=first.camera_center), 3, torch.tensor(pc.BG), pc.step_upstream(i))
        c = float(np.abs(alt["color"] - res["color"]).max()) / hp.COLOR_ATOL
        d0 = pc.step_reference(0)["depth"]
        d = float((np.abs(d0 - res["depth"]) / np.maximum(1.0, np.abs(res["depth"]))).max()) / hp.DEPTH_RTOL
        print(f"[posed] step view {i} ({pc.STEP_POSES[i]}) with view 0's campos: colour {c:.3g} bars; its depth against view 0's: "
              f"{d:.3g} bars")
        assert c >= 100.0 and d >= 100.0, (i, c, d)


# ---- the anti-aliased case ------------------------------------------------------------------------------------------------------
def test_antialiased_case_is_fit_for_the_composed_expectation():
    """As tests/test_aa_cpu.py for its own inputs: coef32 within 1e-5 of coef64 on every visible Gaussian, both sides agree on
    the clamped ones, and the coefficient matters."""
    from tests import aa_cases, aa_ref
    cam, cloud = pc.aa_inputs()
    tfx, tfy = hp.tan_fov(cam)
    c32 = aa_cases.coef_of(cam, cloud, full=True)
    c64 = aa_ref.coef64(cloud["means3D"], cam.world_view_transform, tfx, tfy, cam.image_width, cam.image_height, cloud["scales"],
                        cloud["rotations"], full=True)
    vis = pc.aa_reference()["radii"] > 0
    rel = np.abs(c32["coef"].astype(np.float64) - c64["coef"].numpy()) / c64["coef"].numpy()
    clamped = c32["rho"] <= np.float32(aa_ref.RHO_FLOOR)
    print(f"[posed] antialiased {pc.AA_CASE}: worst relative error of coef32 {rel[vis].max():.3e}, smallest visible coefficient "
          f"{c32['coef'][vis].min():.3f}, clamped and visible {int((vis & clamped).sum())}")
    assert rel[vis].max() <= 1e-5
    assert np.array_equal(clamped[vis], (c64["rho"].numpy() <= aa_ref.RHO_FLOOR)[vis])
    assert int((vis & clamped).sum()) >= 4 and float(c32["coef"][vis].min()) < 0.9


# ---- the restatement against the compiled reference ---------------------------------------------------------------------------
@pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_compiled_reference_bit_for_bit_under_the_pose(case):
    from tests.test_oracle_ref import GRADS, _assert_bit_equal
    cam, cloud, degree = pc.make(case)
    tfx, tfy = hp.tan_fov(cam)
    n = lambda t: t.detach().numpy()
    args = (np.asarray(pc.BG, np.float32), n(cloud["means3D"]), None, n(cloud["opacities"]), n(cloud["scales"]), n(cloud["rotations"]),
            1.0, None, n(cam.world_view_transform), n(cam.full_proj_transform), tfx, tfy, cam.image_height, cam.image_width,
            n(cloud["shs"]), degree, n(cam.camera_center))
    g = n(pc.upstream(cam))
    oracle.set_accum_f32(True)
    ref.set_threads(1)
    try:
        o, r = oracle.forward(*args), ref.forward(*args)
        assert o.num_rendered == r.num_rendered
        for k in ("radii", "color", "depth"):
            _assert_bit_equal(k, getattr(o, k), getattr(r, k))
        so, sr = o.stage(), r.stage()
        vis = r.radii > 0
        for k in ("depths", "means2D", "conic_opacity", "rgb", "clamped"):
            _assert_bit_equal(k, so[k][vis], sr[k][vis])
        for k in ("tiles_touched", "point_list", "point_list_keys", "ranges", "final_T", "n_contrib"):
            _assert_bit_equal(k, so[k], sr[k])
        for name, a, b in zip(GRADS, oracle.backward(o, g), ref.backward(r, g)):
            _assert_bit_equal("dL_d" + name, a, b)
    finally:
        oracle.set_accum_f32(False)
        ref.set_threads(0)
