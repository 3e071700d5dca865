"""CPU: the refusals of lr_views_accumulate, their complete texts and their order.

The step's argument checks are one function (csrc/api.hip check_views_step) that makes no HIP call, so every refusal returns
its code on a machine without a device.  Callers and the other *_cpu tests depend on WHICH refusal a step with several defects
gets, and on which checks an empty step (n_views = 0 or P = 0) still runs.  EXPECTED holds lr_last_error() in full for every
case; the texts were recorded by running these very cases against a build of the commit BEFORE the checks were moved into that
function, and are not taken from the code under test."""
import ctypes
import itertools

import pytest

from tests.test_geom_views_cpu import REJECTED as GEOM_REJECTED
from tests.test_geom_views_cpu import _fake_step as _fake_geom_step
from tests.test_views_args_cpu import REJECTED, TRAIN, _fake_step

NAN, INF = float("nan"), float("inf")
FIXED = dict(dL_dpix="per_view")
STAT_MEMBERS = ("stat_grad_accum", "stat_denom", "stat_max_radii")
PARTIAL_STATS = {"stats_" + "+".join(m[5:] for m in c): dict(FIXED, **{m: "ptr" for m in c})
                 for k in (1, 2) for c in itertools.combinations(STAT_MEMBERS, k)}

# name -> (which fake step, its fields): "args" is lr_views_args (tests/test_views_args_cpu.py), "geom" lr_views_geom_args
CASES = {name: ("args", fields) for name, fields in REJECTED.items()}
CASES.update({"geom_" + name: ("geom", fields) for name, (fields, _) in GEOM_REJECTED.items()})
CASES.update({
    # the geometry refusals the table above does not have
    "geom_inf_distortion_weight": ("geom", dict(TRAIN, distortion_weight=INF)),
    "geom_nan_normal_weight": ("geom", dict(TRAIN, normal_consistency_weight=NAN)),
    "geom_no_rotations": ("geom", dict(TRAIN, out_normals="per_view", rotations=None)),
    "geom_no_acc_scale": ("geom", dict(TRAIN, distortion_weight=1.0, acc_scale=None)),
    "geom_inf_map": ("geom", dict(TRAIN, normal_consistency_weight=1.0, distortion_map=(INF, 0.0, 0.0))),
    "geom_minus_inf_map": ("geom", dict(TRAIN, out_distortion="per_view", distortion_map=(0.0, 0.0, -INF))),
    # the statistics refusals
    "stat_absgrad_alone": ("args", dict(FIXED, stat_absgrad=1)),
    # the depth term's selector
    "bad_depth_loss": ("args", dict(TRAIN, depth_targets="per_view", depth_weight=1.0, depth_loss=7)),
    "pearson_without_depth_targets": ("args", dict(TRAIN, depth_loss=1)),
})
CASES.update({name: ("args", fields) for name, fields in PARTIAL_STATS.items()})

# Steps with two defects: name -> (which fake step, fields, the case of CASES whose refusal comes first in the checks' order)
TWO_DEFECTS = {
    "driver_clash+bad_depth_loss": ("args", dict(TRAIN, dL_dpix="per_view", depth_loss=7), "targets_with_dL_dpix"),
    "precomp+pearson_without_depth": ("args", dict(TRAIN, colors_precomp="ptr", depth_loss=1), "targets_with_colors_precomp"),
    "depth_without_targets+stat_absgrad": ("args", dict(FIXED, depth_targets="per_view", stat_absgrad=1),
                                           "depth_targets_without_targets"),
    "bad_depth_loss+partial_stats": ("args", dict(TRAIN, depth_loss=7, stat_denom="ptr"), "bad_depth_loss"),
    "pearson_without_depth+partial_stats": ("args", dict(TRAIN, depth_loss=1, stat_grad_accum="ptr", stat_denom="ptr"),
                                            "pearson_without_depth_targets"),
    "partial_stats+capacity_zero": ("args", dict(FIXED, stat_grad_accum="ptr", stat_max_radii="ptr", binning_capacity=0),
                                    "stats_grad_accum+max_radii"),
    "stat_absgrad+nan_distortion_weight": ("geom", dict(TRAIN, stat_absgrad=1, distortion_weight=NAN), "stat_absgrad_alone"),
    "negative_normal_weight+no_targets": ("geom", dict(FIXED, normal_consistency_weight=-1.0, out_normals="per_view"),
                                          "geom_negative_normal_weight"),
    "geom_without_targets+no_scales": ("geom", dict(FIXED, distortion_weight=1.0, scales=None), "geom_distortion_without_targets"),
    "no_scales+nan_map": ("geom", dict(TRAIN, out_distortion="per_view", scales=None, distortion_map=(0.0, NAN, 0.0)),
                          "geom_no_scales"),
    "nan_map+negative_depth_weight": ("geom", dict(TRAIN, distortion_weight=1.0, distortion_map=(0.0, NAN, 0.0),
                                                   depth_targets="per_view", depth_weight=-0.5), "geom_nan_map"),
    "negative_depth_weight+no_workspace": ("args", dict(TRAIN, depth_targets="per_view", depth_weight=-0.5, workspace=None),
                                           "negative_depth_weight"),
    "negative_depth_weight+nan_alpha_weight": ("args", dict(TRAIN, depth_targets="per_view", depth_weight=-0.5, masks="per_view",
                                                            alpha_weight=NAN), "negative_depth_weight"),
    "nan_alpha_weight+capacity_zero": ("args", dict(TRAIN, masks="per_view", alpha_weight=NAN, binning_capacity=0),
                                       "nan_alpha_weight"),
    "capacity_zero+no_workspace": ("args", dict(FIXED, binning_capacity=0, workspace=None), "capacity_zero"),
    "no_workspace+no_out_losses": ("args", dict(TRAIN, workspace=None, out_losses=None), "no_workspace"),
    "no_out_losses+acc_mean2D_missing": ("args", dict(TRAIN, out_losses=None, acc_mean2D=None), "targets_without_out_losses"),
    "acc_mean3D_missing+workspace_too_small": ("args", dict(FIXED, acc_mean3D=None, workspace_bytes=4096), "acc_mean3D_missing"),
}

_DRIVERS = "lr_views_accumulate: targets and fixed upstream gradients exclude each other"
_REPRESENTATION = "lr_views_accumulate: targets go with shs and scales / rotations only"
_NEED_TARGETS = "lr_views_accumulate: depth_targets and masks need targets"
_STATS = "lr_views_accumulate: stat_grad_accum, stat_denom and stat_max_radii go together (all three or none)"
_GEOM_WEIGHTS = "distortion_weight and normal_consistency_weight must be finite and >= 0"
_GEOM_TARGETS = "lr_views_accumulate: distortion_weight, normal_consistency_weight, out_distortion and out_normals need targets"
_GEOM_TENSORS = "lr_views_accumulate: the geometry terms need scales, rotations, acc_scale and acc_rot"
_GEOM_MAP = "lr_views_accumulate: distortion_map must be finite"
_DEPTH_WEIGHT = "depth_weight must be finite and >= 0"
_ALPHA_WEIGHT = "alpha_weight must be finite and >= 0"
_CAPACITY = "lr_views_accumulate runs in async mode: binning_capacity > 0 is required"
_ARRAYS = "per-view arrays and workspace are required"
_ACC = "acc_mean2D/acc_opacity/acc_mean3D are required"
_WORKSPACE = "workspace too small (lr_views_workspace_bytes)"
# the complete lr_last_error() of every case of CASES, as recorded (see the module's docstring)
EXPECTED = {
    "targets_with_dL_dpix": _DRIVERS, "targets_with_dL_ddepth": _DRIVERS, "targets_with_dL_dalpha": _DRIVERS,
    "targets_with_colors_precomp": _REPRESENTATION, "targets_with_cov3D_precomp": _REPRESENTATION,
    "targets_with_acc_color": _REPRESENTATION, "targets_with_acc_cov3D": _REPRESENTATION,
    "depth_targets_without_targets": _NEED_TARGETS, "masks_without_targets": _NEED_TARGETS,
    "targets_without_out_losses": "out_losses is required with targets",
    "negative_depth_weight": _DEPTH_WEIGHT, "nan_depth_weight": _DEPTH_WEIGHT, "inf_depth_weight": _DEPTH_WEIGHT,
    "negative_alpha_weight": _ALPHA_WEIGHT, "nan_alpha_weight": _ALPHA_WEIGHT, "bad_depth_weight_with_masks": _DEPTH_WEIGHT,
    "no_driver": _ARRAYS, "capacity_zero": _CAPACITY, "no_workspace": _ARRAYS,
    "workspace_too_small": _WORKSPACE, "workspace_too_small_train": _WORKSPACE,
    "acc_mean2D_missing": _ACC, "acc_opacity_missing": _ACC, "acc_mean3D_missing": _ACC, "viewmatrices_missing": _ARRAYS,
    "geom_negative_distortion_weight": _GEOM_WEIGHTS, "geom_nan_distortion_weight": _GEOM_WEIGHTS,
    "geom_inf_distortion_weight": _GEOM_WEIGHTS, "geom_inf_normal_weight": _GEOM_WEIGHTS,
    "geom_negative_normal_weight": _GEOM_WEIGHTS, "geom_nan_normal_weight": _GEOM_WEIGHTS,
    "geom_distortion_without_targets": _GEOM_TARGETS, "geom_normal_term_without_targets": _GEOM_TARGETS,
    "geom_maps_without_targets": _GEOM_TARGETS,
    "geom_nan_map": _GEOM_MAP, "geom_inf_map": _GEOM_MAP, "geom_minus_inf_map": _GEOM_MAP,
    "geom_no_acc_rot": _GEOM_TENSORS, "geom_no_acc_scale": _GEOM_TENSORS, "geom_no_scales": _GEOM_TENSORS,
    "geom_no_rotations": _GEOM_TENSORS, "geom_workspace": _WORKSPACE,
    "stats_grad_accum": _STATS, "stats_denom": _STATS, "stats_max_radii": _STATS, "stats_grad_accum+denom": _STATS,
    "stats_grad_accum+max_radii": _STATS, "stats_denom+max_radii": _STATS,
    "stat_absgrad_alone": "lr_views_accumulate: stat_absgrad needs stat_grad_accum, stat_denom and stat_max_radii",
    "bad_depth_loss": "lr_views_accumulate: depth_loss must be LR_DEPTH_LOSS_L1 or LR_DEPTH_LOSS_PEARSON",
    "pearson_without_depth_targets": "lr_views_accumulate: depth_loss needs depth_targets",
}
# The refusals an empty step never reaches (it returns 0 in front of them); every other case of CASES is refused all the same.
BEHIND_THE_EMPTY_RETURN = {
    "targets_without_out_losses", "no_driver", "capacity_zero", "no_workspace", "workspace_too_small", "workspace_too_small_train",
    "acc_mean2D_missing", "acc_opacity_missing", "acc_mean3D_missing", "viewmatrices_missing", "geom_workspace"}


@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


def _step(kind, fields):
    return (_fake_geom_step if kind == "geom" else _fake_step)(**fields)


def _refusal(L, a):
    """(return code, complete message) of the step; the message of a call that returns 0 is not defined."""
    rc = L.lr_views_accumulate(a)
    return rc, (L.lr_last_error().decode() if rc != 0 else None)


def test_the_tables_cover_what_they_claim():
    assert set(EXPECTED) == set(CASES)
    assert set(REJECTED) <= set(CASES) and {"geom_" + n for n in GEOM_REJECTED} <= set(CASES)
    assert len(PARTIAL_STATS) == 6 and len(TWO_DEFECTS) >= 8
    assert BEHIND_THE_EMPTY_RETURN < set(CASES)
    assert all(first in CASES for _, _, first in TWO_DEFECTS.values())


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal_has_its_complete_text(L, case):
    from luciddreamer_amd import _lib
    assert _refusal(L, _step(*CASES[case])) == (_lib.LR_ERR_INVALID_ARG, EXPECTED[case])


@pytest.mark.parametrize("which", ["targets", "depth_targets", "masks"])
def test_null_entry_has_its_complete_text_and_its_place(L, which):
    """Behind the weights (a NaN alpha_weight wins), in front of the empty return's checks (capacity 0 loses); the entries are
    read for a step with views and Gaussians only."""
    from luciddreamer_amd import _lib
    full = dict(TRAIN, depth_targets="per_view", depth_weight=1.0, masks="per_view", alpha_weight=1.0)
    for fields, want in ((full, "NULL entry in targets / depth_targets / masks"), (dict(full, alpha_weight=NAN), _ALPHA_WEIGHT),
                         (dict(full, binning_capacity=0), "NULL entry in targets / depth_targets / masks")):
        a = _fake_step(**fields)
        holed = (ctypes.c_void_p * 2)(a.background, None)
        setattr(a, which, ctypes.addressof(holed))
        assert _refusal(L, a) == (_lib.LR_ERR_INVALID_ARG, want)
        a.P = 0
        assert _refusal(L, a) == ((_lib.LR_ERR_INVALID_ARG, want) if want == _ALPHA_WEIGHT else (0, None))


@pytest.mark.parametrize("case", sorted(TWO_DEFECTS))
def test_the_earlier_check_wins(L, case):
    from luciddreamer_amd import _lib
    kind, fields, first = TWO_DEFECTS[case]
    assert _refusal(L, _step(kind, fields)) == (_lib.LR_ERR_INVALID_ARG, EXPECTED[first])


@pytest.mark.parametrize("empty", ["n_views", "P"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_empty_step_runs_the_checks_in_front_of_its_return_only(L, case, empty):
    from luciddreamer_amd import _lib
    a = _step(*CASES[case])
    setattr(a, empty, 0)
    want = (0, None) if case in BEHIND_THE_EMPTY_RETURN else (_lib.LR_ERR_INVALID_ARG, EXPECTED[case])
    assert _refusal(L, a) == want


@pytest.mark.parametrize("empty", ["n_views", "P"])
@pytest.mark.parametrize("case", sorted(TWO_DEFECTS))
def test_empty_step_with_two_defects(L, case, empty):
    """The first defect of each of these steps sits in front of the empty return, except where it is one of
    BEHIND_THE_EMPTY_RETURN: then so does the second, and the step returns 0."""
    from luciddreamer_amd import _lib
    kind, fields, first = TWO_DEFECTS[case]
    a = _step(kind, fields)
    setattr(a, empty, 0)
    want = (0, None) if first in BEHIND_THE_EMPTY_RETURN else (_lib.LR_ERR_INVALID_ARG, EXPECTED[first])
    assert _refusal(L, a) == want
