"""The conditions of the camera-intrinsics GPU tests (tests/test_gpu_intrinsics.py), checked where there is no GPU, on the very
cases of tests/intrinsics_cases.py: the camera builder reproduces cameras.make_camera bit for bit where it should, the CPU
oracle flags no pixel of any reference the GPU tests compare with (gradients are held to the whole-tensor bar), no case is
trivial, the two CPU references agree under every intrinsics row, every case differs by at least 100 times the GPU test's bar
when the intrinsics are altered on the reference side the way a wrong kernel would alter them, and znear / zfar do not reach the
outputs."""
import math

import numpy as np
import pytest
import torch

from luciddreamer_amd import cameras
from tests import helpers as hp, intrinsics_cases as ic, posed_cases as pc
from tests.test_posed_cases_cpu import _float64
from tests.test_screen_cull_cpu import sc              # noqa: F401 -- the host build of csrc/screen_cull.h, as a fixture

CASES = list(ic.CASES)


def _flag_counts(res):
    fr = res["res"].stage()["fragile"]
    return int((fr != 0).sum()), int(((fr & 1) != 0).sum()), int(((fr & 2) != 0).sum())


# ---- the camera builder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", ["translated", "general"])
@pytest.mark.parametrize("W,H", [(97, 61), (160, 96), (96, 112)])
def test_camera_reproduces_make_camera_bit_for_bit(pose, W, H):
    """shift = (0, 0) and the aspect-derived tangents: cameras.make_camera's own matrices."""
    want = pc.camera(pose, W, H)
    tan_x = math.tan(0.5 * cameras.FOVX_DEFAULT)
    tan_y = math.tan(0.5 * cameras.fovy_from_fovx(cameras.FOVX_DEFAULT, W, H))
    got = ic.camera(pose, W, H, tan_x, tan_y)
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    assert (got.image_width, got.image_height, got.znear, got.zfar) == (W, H, want.znear, want.zfar)
    # the tangents the kernels are handed are floats: the same bits
    assert np.array_equal(np.float32(hp.tan_fov(got)), np.float32(hp.tan_fov(want)))


def test_camera_entries_are_what_the_table_says():
    for case in CASES:
        W, H, tx, ty, shift, pose, zn, zf = ic.INTRINSICS[case][:8]
        tx, ty = ic.tangents(case)
        cam = ic.make(case)[0]
        P = (torch.inverse(cam.world_view_transform.double()) @ cam.full_proj_transform.double()).T
        want = ic.projection(tx, ty, shift, zn, zf).double()
        assert float((P - want).abs().max()) <= 1e-5 * float(want.abs().max()), case
        got = hp.tan_fov(cam)
        assert abs(got[0] - tx) <= 1e-12 and abs(got[1] - ty) <= 1e-12, case
        assert torch.equal(cam.world_view_transform, pc.camera(pose, W, H).world_view_transform)
    assert sorted({ic.INTRINSICS[c][8] for c in CASES}) == [0, 1, 2, 3]           # every SH degree is among the rows


# ---- the references are fit for their comparisons -----------------------------------------------------------------------------
def _every_reference():
    """(label, helpers.run_oracle result, image pixels) of every oracle run the GPU tests compare with."""
    for case in CASES:
        cam = ic.make(case)[0]
        yield case, ic.reference(case), cam.image_width * cam.image_height
    cam = ic.precomp_inputs()[0]
    yield "precomp " + ic.PRECOMP_CASE, ic.precomp_reference(), cam.image_width * cam.image_height
    for case in ic.RAW_CASES:
        cam = ic.make(case)[0]
        yield "raw " + case, ic.raw_reference(case), cam.image_width * cam.image_height
    cam, _ = ic.aa_inputs()
    yield "antialiased " + ic.AA_CASE, ic.aa_reference(), cam.image_width * cam.image_height
    cams, _ = ic.step_scene()
    for i, (pose, row) in enumerate(ic.STEP_VIEWS):
        yield f"step view {i} ({pose}, {row})", ic.step_reference(i), cams[i].image_width * cams[i].image_height


def test_flagged_pixels_stay_within_the_caps():
    """helpers.compare_forward caps the colour-flagged pixels at max(8, FRAGILE_FRAC pixels); every gradient comparison of the
    GPU tests is helpers.compare_grads (the whole tensor), so no reference may hold a flagged pixel of either kind."""
    for label, res, pixels in _every_reference():
        any_, colour, depth = _flag_counts(res)
        print(f"[intrinsics] {label}: flagged pixels {any_} (colour {colour}, depth {depth}) of {pixels}, "
              f"{int((res['radii'] > 0).sum())} visible of {res['radii'].size}")
        assert colour <= max(8, hp.FRAGILE_FRAC * pixels), label
        assert any_ == 0, label


def _beyond_clamp(cam, cloud, visible):
    """Visible Gaussians whose view-space x / z (y / z) lies beyond the 1.3 tan clamp of the Jacobian, per axis."""
    V = cam.world_view_transform.double()
    p = cloud["means3D"].double() @ V[:3, :3] + V[3, :3]
    tx, ty = hp.tan_fov(cam)
    vis = torch.from_numpy(visible)
    return (int((vis & ((p[:, 0] / p[:, 2]).abs() > 1.3 * tx)).sum()), int((vis & ((p[:, 1] / p[:, 2]).abs() > 1.3 * ty)).sum()))


@pytest.mark.parametrize("case", CASES)
def test_case_is_not_trivial(sc, case):              # noqa: F811
    W, H, _, ty_row, shift = ic.INTRINSICS[case][:5]
    cam, cloud, _ = ic.make(case)
    res = ic.reference(case)
    visible = res["radii"] > 0
    P = visible.size
    Pm = cam.full_proj_transform.numpy().reshape(-1)              # Pm[k] as the kernels index it
    tx, ty = hp.tan_fov(cam)
    ratio = (W / (2 * tx)) / (H / (2 * ty))
    nx, ny = _beyond_clamp(cam, cloud, visible)
    near, rej = sc(cloud, cam)
    print(f"[intrinsics] {case}: {int(visible.sum())} visible of {P}; focal_x / focal_y {ratio:.3f}; Pm[8] {Pm[8]:.3f}, Pm[9] "
          f"{Pm[9]:.3f}; visible beyond the clamp: x {nx}, y {ny}; pooled off-screen test: {int((near & rej).sum())} rejected, "
          f"{int((near & ~rej).sum())} passed")
    assert visible.sum() >= 0.4 * P
    if any(shift):
        assert abs(Pm[8]) > 0.1 and abs(Pm[9]) > 0.1
    elif ic.INTRINSICS[case][5] == "translated":                  # (a turned view matrix puts its own terms there)
        assert Pm[8] == 0 and Pm[9] == 0
    if case in ("tall_pixels", "wide_pixels"):                    # the rows that isolate non-square pixels
        assert not 0.6 <= ratio <= 1.6
    elif ty_row is not None:
        # general: 0.62 and 0.27 at 131 x 77 are focal_x / focal_y = 0.74, a quarter off square; that this is far enough is
        # what test_case_is_sensitive_to_the_intrinsics_bugs_it_aims_at shows ("square": above 2000 bars in every tensor)
        assert not 0.8 <= ratio <= 1.25
    else:
        assert abs(ratio - 1.0) < 1e-6
    if case in ic.CLAMP_CASES:
        assert nx >= 10 and ny >= 10
    assert (near & rej).sum() > 0 and (near & ~rej).sum() > 0
    assert not (rej & near & visible).any()                       # (what tests/test_screen_cull_cpu.py holds it to)


def test_step_views_mix_poses_and_intrinsics():
    cams, _ = ic.step_scene()
    rows = [r for _, r in ic.STEP_VIEWS]
    assert len(set(rows)) == 5 and len({p for p, _ in ic.STEP_VIEWS}) == 5 and rows != sorted(rows)
    assert len({hp.tan_fov(c) for c in cams}) == 5
    assert all((c.image_width, c.image_height) == ic.STEP_SCENE[1:3] for c in cams)
    for i in range(len(cams)):
        assert int((ic.step_reference(i)["radii"] > 0).sum()) >= 100, i


@pytest.mark.parametrize("case", CASES)
def test_c_oracle_and_float64_restatement_agree_under_the_intrinsics(case):
    """As tests/test_posed_cases_cpu.py: colour and depth 1e-5, gradients helpers.GRAD_RTOL of each tensor's maximum."""
    cam, cloud, degree = ic.make(case)
    res = ic.reference(case)
    col, dep, radii, grads = _float64(cam, cloud, degree, ic.upstream(cam))
    assert np.array_equal(radii, res["radii"])
    c_err = float(np.abs(res["color"] - col).max())
    d_err = float((np.abs(res["depth"] - dep) / np.maximum(1.0, np.abs(dep))).max())
    figures = {}
    for k in ic.NAMES_SH:
        b = grads[k]
        figures[k] = (float(np.abs(res["grads"][k].reshape(b.shape) - b).max()), float(np.abs(b).max()))
    print(f"[intrinsics] {case}: C oracle vs float64: colour {c_err:.2e}, depth (relative) {d_err:.2e}, gradients (of each "
          "maximum) " + ", ".join(f"{k} {e / s:.2e}" for k, (e, s) in figures.items()))
    assert c_err <= 1e-5 and d_err <= 1e-5
    for k, (e, s) in figures.items():
        assert s > 0, k
        assert e <= hp.GRAD_RTOL * s, (k, e, s)


# ---- sensitivity: the GPU tests would fail on a kernel that is wrong in one of these ways --------------------------------------
def _distances(res, alt):
    """Each difference as a multiple of the bar the GPU test applies to that quantity."""
    out = {"colour": float(np.abs(alt["color"] - res["color"]).max()) / hp.COLOR_ATOL}
    for k in ic.NAMES_SH:
        scale = float(np.abs(res["grads"][k]).max())
        out[k] = float(np.abs(alt["grads"][k] - res["grads"][k]).max()) / (hp.GRAD_RTOL * scale)
    return out


@pytest.mark.parametrize("case", CASES)
def test_case_is_sensitive_to_the_intrinsics_bugs_it_aims_at(case):
    cam, cloud, degree = ic.make(case)
    res = ic.reference(case)
    for how in ic.aims(case):
        alt = hp.run_oracle(cloud, ic.altered(cam, how), degree, torch.tensor(ic.BG), ic.upstream(cam))
        ratios = _distances(res, alt)
        print(f"[intrinsics] {case}, {how}: difference / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) +
              f"; radii changed on {int((alt['radii'] != res['radii']).sum())} Gaussians")
        assert ratios["colour"] >= 100.0, (case, how, ratios)
        assert max(v for k, v in ratios.items() if k != "colour") >= 100.0, (case, how, ratios)


def test_every_alteration_is_aimed_at():
    for how in ("square", "swapped"):
        assert {c for c in CASES if how in ic.aims(c)} == {"tall_pixels", "wide_pixels", "general"}
    assert {c for c in CASES if "centred" in ic.aims(c)} == {"off_centre", "general"}
    assert not ic.aims("wide") and not ic.aims("narrow")          # (these two aim at the clamp and the cull bound)


def test_step_views_differ_from_view_0s_tangents_by_far_more_than_the_bar():
    """A step that read view 0's tangents for every view would have to fail on every other view."""
    cams, cloud = ic.step_scene()
    for i in range(1, len(cams)):
        res = ic.step_reference(i)
        alt = hp.run_oracle(cloud, ic.altered(cams[i], "first_view"), 3, torch.tensor(ic.BG), ic.step_upstream(i))
        ratios = _distances(res, alt)
        print(f"[intrinsics] step view {i} {ic.STEP_VIEWS[i]} with view 0's tangents: difference / bar: " +
              ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
        assert ratios["colour"] >= 100.0, (i, ratios)
        assert max(v for k, v in ratios.items() if k != "colour") >= 100.0, (i, ratios)


# ---- near and far ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_znear_and_zfar_do_not_reach_the_outputs(case):
    """The kernels never read the third clip row, and neither does the oracle: another near / far pair, the same bits."""
    cam, cloud, degree = ic.make(case)
    res = ic.reference(case)
    zn, zf = (0.01, 100.0) if cam.znear == 0.5 else (0.5, 20.0)
    other = ic.row_camera(case, znear=zn, zfar=zf)
    assert not torch.equal(other.full_proj_transform, cam.full_proj_transform)
    assert torch.equal(other.full_proj_transform[:, [0, 1, 3]], cam.full_proj_transform[:, [0, 1, 3]])
    alt = hp.run_oracle(cloud, other, degree, torch.tensor(ic.BG), ic.upstream(cam))
    for k in ("color", "depth", "radii"):
        assert np.array_equal(alt[k], res[k]), k
    for k in ic.NAMES_SH:
        assert np.array_equal(alt["grads"][k], res["grads"][k]), k


# ---- the anti-aliased case ------------------------------------------------------------------------------------------------------
def test_antialiased_case_is_fit_for_the_composed_expectation():
    """As tests/test_posed_cases_cpu.py for its own inputs: coef32 within 1e-5 of coef64 on every visible Gaussian, both sides
    agree on the clamped ones, and the coefficient matters."""
    from tests import aa_cases, aa_ref
    cam, cloud = ic.aa_inputs()
    tfx, tfy = hp.tan_fov(cam)
    c32 = aa_cases.coef_of(cam, cloud, full=True)
    c64 = aa_ref.coef64(cloud["means3D"], cam.world_view_transform, tfx, tfy, cam.image_width, cam.image_height, cloud["scales"],
                        cloud["rotations"], full=True)
    vis = ic.aa_reference()["radii"] > 0
    rel = np.abs(c32["coef"].astype(np.float64) - c64["coef"].numpy()) / c64["coef"].numpy()
    clamped = c32["rho"] <= np.float32(aa_ref.RHO_FLOOR)
    print(f"[intrinsics] antialiased {ic.AA_CASE}: worst relative error of coef32 {rel[vis].max():.3e}, smallest visible "
          f"coefficient {c32['coef'][vis].min():.3f}, clamped and visible {int((vis & clamped).sum())}")
    assert rel[vis].max() <= 1e-5
    assert np.array_equal(clamped[vis], (c64["rho"].numpy() <= aa_ref.RHO_FLOOR)[vis])
    assert int((vis & clamped).sum()) >= 4 and float(c32["coef"][vis].min()) < 0.9
