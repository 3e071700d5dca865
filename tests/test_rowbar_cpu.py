"""The per-row gradient bar on the CPU (tests/rowbar.py, tests/rowbar_cases.py): no GPU.

1. The gap, as a test: gradients that are wrong in a small term or in small rows pass helpers.compare_grads (the tensor-wide bar
   every gradient check of the rasterizer used) and are rejected by row_bar.
2. The references alone stay inside the bar: on every case the C oracle passes row_bar calibrated by the float32 torch run, and
   the reverse, with no row excused -- the condition that keeps tests/test_gpu_rowbar.py honest, checked before a GPU is involved.
3. Every case has the rows it is there for.
4. row_bar itself."""
import numpy as np
import pytest
import torch

from oracle import torch_oracle
from tests import helpers as hp, rowbar as rb, rowbar_cases as rc


# ---- 1. the gap -------------------------------------------------------------------------------------------------------------
def _means3D_without_direction_term(name):
    """Float64 dL/dmeans3D of the same scene with its colours passed as colors_precomp: everything but the chain through the view
    direction of the SH evaluation."""
    case = rc.make(name)
    cam = case["cam"]
    lv = rc._leaves(case, torch.float64)
    d = lv["means3D"].detach() - cam.camera_center.double()[None, :]
    rgb = torch_oracle.sh_to_rgb(case["degree"], lv["sh"].detach(), d / d.norm(dim=1, keepdim=True))
    tfx, tfy = hp.tan_fov(cam)
    col, _, _ = torch_oracle.render(lv["means3D"], lv["opacity"], cam.world_view_transform, cam.full_proj_transform,
                                    cam.camera_center, tfx, tfy, cam.image_height, cam.image_width, torch.tensor(rc.BG),
                                    scales=lv["scales"], rotations=lv["rotations"], colors_precomp=rgb, means2D=lv["means2D"])
    (col * case["g_color"].double()).sum().backward()
    return lv["means3D"].grad.numpy()


def _accepted_by_the_tensor_bar(mutant, ref, k):
    try:
        hp.compare_grads({k: mutant}, {k: ref[k]}, names=[k])
    except AssertionError:
        return False
    return True


def _mutants(name):
    """(kind, what, tensor, array) built from the float64 gradients of a case: the SH-direction term of dL/dmeans3D scaled by
    0.998 ("term"), and per tensor the rows below 1e-4 of the tensor maximum set to zero ("rows")."""
    ref = rc.torch_grads(name)
    term = ref["means3D"] - _means3D_without_direction_term(name)
    assert np.abs(term).max() > 1e-3 * np.abs(ref["means3D"]).max()       # the term exists (SH degree 3)
    out = [("term", "direction term x 0.998", "means3D", ref["means3D"] - 0.002 * term)]
    for k in rc.make(name)["names"]:
        row_max = np.abs(ref[k].reshape(ref[k].shape[0], -1)).max(axis=1)
        small = (row_max > 0) & (row_max < 1e-4 * row_max.max())
        if small.any():
            m = ref[k].copy()
            m[small] = 0.0
            out.append(("rows", f"{int(small.sum())} small rows zeroed", k, m))
    return out


def test_wrong_small_terms_and_rows_pass_the_tensor_bar_and_fail_the_row_bar():
    """Observed.  sparse_deg3: the direction term x 0.998 moves dL/dmeans3D by 2.3e-05 of the tensor maximum, compare_grads
    ACCEPTS it, row_bar rejects 34 rows; 1 or 2 small rows zeroed in means2D, means3D, scales, rotations (1.5e-06 to 8.3e-05):
    accepted every time, every zeroed row rejected by row_bar.  occluded: the same term is a larger share there (1.4e-04,
    compare_grads rejects it too; row_bar rejects 114 rows); 6 to 16 small rows zeroed in each of the six tensors (5.0e-05 to
    9.8e-05): accepted every time, every zeroed row rejected."""
    accepted = {"term": [], "rows": []}
    for name in ("sparse_deg3", "occluded"):
        ref = rc.torch_grads(name)
        cals = [rc.c_oracle(name)["grads"], rc.torch_grads(name, torch.float32)]
        kinds = set()
        for kind, what, k, m in _mutants(name):
            acc = _accepted_by_the_tensor_bar(m, ref, k)
            rep = rb.judge(m, ref[k], [c[k] for c in cals])
            err = np.abs(m - ref[k]).max() / np.abs(ref[k]).max()
            print(f"[rowbar] {name}: {what} in {k}: {err:.1e} of the tensor maximum, compare_grads "
                  f"{'ACCEPTS' if acc else 'rejects'}, row_bar rejects {len(rep['failed'])} rows")
            assert rep["failed"], (name, what, k)                             # row_bar rejects every one of them
            if kind == "rows":
                assert len(rep["failed"]) == int(what.split()[0]), (name, what, k)
            accepted[kind].append(acc)
            kinds.add(kind)
        assert kinds == {"term", "rows"}, name                                # both kinds of mutant exist on either case
        # and the unmutated reference's own restatements pass what the mutants fail
        for k in rc.make(name)["names"]:
            rb.row_bar(cals[0][k], ref[k], [cals[1][k]], what=f"{name} {k}")
    for kind, acc in accepted.items():
        assert any(acc), f"the tensor bar accepts no mutant of the kind '{kind}': the seeds do not show the gap"
    assert all(accepted["rows"])


# ---- 2. the references alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.NAMES)
def test_references_alone_stay_inside_the_bar_with_no_row_excused(name):
    case = rc.make(name)
    ref, t32, c = rc.torch_grads(name), rc.torch_grads(name, torch.float32), rc.c_oracle(name)["grads"]
    a = rb.check_all(c, ref, [t32], case["names"], fragile_rows=None, what=f"{name}: C oracle, calibrated by torch float32")
    b = rb.check_all(t32, ref, [c], case["names"], fragile_rows=None, what=f"{name}: torch float32, calibrated by the C oracle")
    for rep in list(a.values()) + list(b.values()):
        assert rep["excused"] == [] and rep["failed"] == []
    # a flip of a discrete decision between float64 and BOTH float32 runs would pass the above and leave the bar meaningless
    # on that row: no row is further than 1e-2 of itself from the float64 reference
    assert max(r["worst"] for r in list(a.values()) + list(b.values())) < 1e-2


# ---- 3. the cases ------------------------------------------------------------------------------------------------------------
def test_cases_are_small_and_one_is_ragged():
    ragged = 0
    for name in rc.NAMES:
        cam, P = rc.make(name)["cam"], rc.make(name)["cloud"]["means3D"].shape[0]
        assert P <= 400 and cam.image_width <= 96 and cam.image_height <= 80, name
        ragged += cam.image_width % 16 != 0 and cam.image_height % 16 != 0
    assert ragged >= 1


def _rel_row_max(g):
    m = np.abs(g.reshape(g.shape[0], -1)).max(axis=1)
    return m / m.max()


def test_cases_have_the_rows_they_are_there_for():
    # sparse: rows between 2e-4 and 1e-2 of the tensor maximum
    r = _rel_row_max(rc.torch_grads("sparse_deg3")["means3D"])
    assert int(((r > 0) & (r < 1e-2)).sum()) >= 10
    # degree 0: no direction term at all
    ref = rc.torch_grads("sparse_deg0")["means3D"]
    assert np.abs(ref - _means3D_without_direction_term("sparse_deg0")).max() <= 1e-12 * np.abs(ref).max()
    # occluded: rows at 1e-4 of the tensor maximum and below, in every tensor
    for k, g in rc.torch_grads("occluded").items():
        r = _rel_row_max(g)
        assert int(((r > 0) & (r < 1e-4)).sum()) >= 5, k
    # posed: no entry of the view matrix's upper 4 x 3 is trivial
    V = rc.make("posed")["cam"].world_view_transform
    assert float(V[:4, :3].abs().min()) > 0.05
    # fov_clamp: Gaussians beyond the clamp in x only and in y only that reach the image
    case = rc.make("fov_clamp")
    g = np.abs(rc.torch_grads("fov_clamp")["means3D"]).max(axis=1)
    x_only, y_only = rc.clamp_classes(case)
    assert int((x_only & (g > 0)).sum()) >= 5 and int((y_only & (g > 0)).sum()) >= 5
    # sh_clamp: visible rows with a channel whose colour is clamped (zero dL/dsh in that channel, not in another)
    sh = np.abs(rc.torch_grads("sh_clamp")["sh"]).max(axis=1)            # (P, 3)
    assert int(((sh == 0).any(axis=1) & (sh > 0).any(axis=1)).sum()) >= 20
    # precomp / scale_modifier: the tensors and the modifier
    assert rc.make("precomp")["names"] == rc.NAMES_PRE and rc.make("scale_modifier")["scale_modifier"] == 1.7
    assert np.abs(rc.torch_grads("precomp")["cov3D"]).max() > 0 and np.abs(rc.torch_grads("precomp")["colors"]).max() > 0
    # long_lists: lists longer than a segment of the blend backward, which the other cases never reach; rows that are exactly zero
    # (hidden behind T < 1e-4) and rows below 1e-4 of the tensor maximum
    assert int((rc.list_lengths("long_lists") > 256).sum()) >= 3 and int(rc.list_lengths("occluded").max()) <= 256
    g = np.abs(rc.torch_grads("long_lists")["means3D"]).max(axis=1)
    assert int((g == 0).sum()) >= 10 and int(((g > 0) & (g < 1e-4 * g.max())).sum()) >= 50
    # constant_upstream: every splat wholly on screen, and the position gradient is what is left of a cancellation: for the
    # typical row more than half of the magnitudes summed over the pixels cancels in the signed sum (observed: median 0.31)
    case, c = rc.make("constant_upstream"), rc.c_oracle("constant_upstream")
    m2, rad = c["res"].stage()["means2D"], c["radii"]
    assert (rad > 0).all()
    assert (m2[:, 0] - rad >= 0).all() and (m2[:, 0] + rad <= case["cam"].image_width - 1).all()
    assert (m2[:, 1] - rad >= 0).all() and (m2[:, 1] + rad <= case["cam"].image_height - 1).all()
    a, s = rc.abs_reference("constant_upstream")
    assert np.median(np.abs(s).max(axis=1) / a.max(axis=1)) < 0.5


def test_scale_gradient_is_with_respect_to_the_modified_scale():
    """The convention of the reference's backward, kept by the C oracle and the kernels: dL/dscales under a scale modifier is
    dL/d(mod * s).  The true derivative with respect to s is mod times that."""
    case = rc.make("scale_modifier")
    lv = {k: case["cloud"][k].double().clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    cam = case["cam"]
    tfx, tfy = hp.tan_fov(cam)
    col, _, _ = torch_oracle.render(lv["means3D"], lv["opacities"], cam.world_view_transform, cam.full_proj_transform,
                                    cam.camera_center, tfx, tfy, cam.image_height, cam.image_width, torch.tensor(rc.BG),
                                    scales=lv["scales"], rotations=lv["rotations"], scale_modifier=1.7, shs=lv["shs"], degree=2)
    (col * case["g_color"].double()).sum().backward()
    ref = rc.torch_grads("scale_modifier")
    np.testing.assert_allclose(lv["scales"].grad.numpy(), 1.7 * ref["scales"], rtol=1e-9, atol=1e-12 * np.abs(ref["scales"]).max())
    np.testing.assert_allclose(lv["rotations"].grad.numpy(), ref["rotations"], rtol=1e-9, atol=1e-12 * np.abs(ref["rotations"]).max())


def test_absgrad_reference_sums_to_the_signed_gradient_and_float32_stays_at_the_floor():
    """One backward through grad_oracle's pixel_probe instead of tests/absgrad_ref.py's one per pixel: the signed sum of the shares
    is the whole-image dL/dmeans2D, and -- all-positive sums, no cancellation -- the float32 evaluation is within the floor
    GRAD_RTOL * row_max on every row (observed: worst 2.2e-06 of the row)."""
    a64, s64 = rc.abs_reference("occluded")
    g = rc.torch_grads("occluded")["means2D"]
    assert np.abs(s64 - g[:, :2]).max() <= 1e-12 * np.abs(g).max()
    assert (a64 >= np.abs(s64) * (1 - 1e-12)).all() and int((a64.max(axis=1) > 0).sum()) > 250
    a32, _ = rc.abs_reference("occluded", torch.float32)
    rep = rb.row_bar(a32, a64, [a32], what="absgrad float32")
    print(f"[rowbar] absgrad, float32 against float64: worst {rep['worst']:.1e}, rows above the floor {rep['above_floor']}")
    assert rep["above_floor"] == 0


def test_multi_view_scene_has_rows_visible_in_one_view_only():
    vis = np.stack([rc.c_oracle(rc.VIEW_CASE, None, v)["radii"] > 0 for v in range(len(rc.VIEW_POSES))])
    assert (vis.sum(axis=1) > 100).all()
    assert int((vis.sum(axis=0) == 1).sum()) >= 50


# ---- 4. row_bar itself -------------------------------------------------------------------------------------------------------
def _toy():
    ref = np.array([[1.0, -2.0], [1e-6, 3e-6], [0.0, 0.0], [5.0, 0.0]])
    return ref, ref.astype(np.float32).astype(np.float64)


def test_row_bar_holds_every_row_to_its_own_scale():
    ref, cal = _toy()
    got = ref.copy()
    got[1] *= 1.0 + 5e-5                                                   # inside 1e-4 of the row
    assert rb.row_bar(got, ref, [cal])["failed"] == []
    got[1, 1] = 3e-6 * 1.01                                                # 1 % of a row that is 6e-7 of the tensor maximum
    hp.compare_grads({"t": got}, {"t": ref}, names=["t"])                  # the tensor bar does not see it
    rep = rb.judge(got, ref, [cal])
    assert [i for i, _ in rep["failed"]] == [1] and rep["above_floor"] == 1
    with pytest.raises(AssertionError, match="outside the per-row bar"):
        rb.row_bar(got, ref, [cal], what="toy")


def test_row_bar_calibrator_arm_and_margin():
    ref, cal = _toy()
    cal = cal.copy()
    cal[0, 1] += 1e-3                                                      # float32 is off by 5e-4 of row 0
    got = ref.copy()
    got[0, 1] += 3.9e-3
    assert rb.judge(got, ref, [ref, cal])["failed"] == []                  # the largest distance of ANY calibrator, times 4
    got[0, 1] += 0.2e-3
    assert [i for i, _ in rb.judge(got, ref, [ref, cal])["failed"]] == [0]


def test_row_bar_zero_rows_and_all_zero_rows():
    ref, cal = _toy()
    got = ref.copy()
    got[2, 0] = 1e-30                                                      # the reference row is zero: exactly zero
    assert [i for i, _ in rb.judge(got, ref, [cal])["failed"]] == [2]
    got = ref.copy()
    got[1] = 0.0                                                           # all zero where the reference is not: whatever its size
    loose = ref.copy()
    loose[1] = 0.0                                                         # even if a calibrator were as wrong
    assert [i for i, _ in rb.judge(got, ref, [loose])["failed"]] == [1]
    got = ref.copy()
    got[3, 0] = np.nan
    assert [i for i, _ in rb.judge(got, ref, [cal])["failed"]] == [3]


def test_row_bar_fragile_excuse_granted_and_refused():
    ref = np.arange(1.0, 11.0).reshape(5, 2)
    got = ref.copy()
    got[[1, 3]] *= 1.01
    rep = rb.row_bar(got, ref, [ref], fragile_rows={1, 3, 4})              # granted: both touch a flagged pixel
    assert rep["excused"] == [1, 3] and rep["failed"] == []
    rep = rb.judge(got, ref, [ref], fragile_rows={3})                      # refused: row 1 touches none
    assert rep["excused"] == [3] and [i for i, _ in rep["failed"]] == [1]
    got[4] *= 1.01                                                         # refused: a third row would need the excuse
    rep = rb.judge(got, ref, [ref], fragile_rows={1, 3, 4})
    assert rep["excused"] == [1, 3] and [i for i, _ in rep["failed"]] == [4]
    with pytest.raises(AssertionError):
        rb.row_bar(got, ref, [ref], fragile_rows={1, 3, 4})


def test_fragile_rows_are_those_of_compare_grads_by_row():
    """rowbar.fragile_rows_of uses helpers.touches_fragile, the rule factored out of helpers.compare_grads_by_row: on a scene with
    flagged pixels the set is not empty, holds visible rows only, and a scene without flagged pixels has none."""
    from luciddreamer_amd import synthetic
    found = None
    for seed in range(1, 8):
        cam, cloud = hp.box_setup(300, 64, 64, seed, scale_mult=3.0)
        c = hp.run_oracle(cloud, cam, 3, torch.tensor(rc.BG), synthetic.upstream_grad(64, 64))
        if (c["res"].stage()["fragile"] != 0).any():
            found = c
            break
    assert found is not None
    rows = rb.fragile_rows_of(found)
    assert len(rows) >= 1 and all(found["radii"][i] > 0 for i in rows)
    assert len(rows) < int((found["radii"] > 0).sum())
    assert rb.fragile_rows_of(rc.c_oracle("sparse_deg3")) == frozenset()
