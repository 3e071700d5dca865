"""Absolute view-space gradient (AbsGS; config.set_absgrad, lr_backward_args::dL_dmean2D_abs): the contract's CPU
side -- the float64 reference checks itself, the seeded cases are fit for the GPU comparisons, the switch and the exports."""
import os
import re

import numpy as np
import pytest

from tests import absgrad_cases as cases
from tests import absgrad_ref as ref

DISTINCT = [n for n in cases.NAMES if n != "partial_strict"]       # "partial_strict" shares the reference of "partial"


@pytest.mark.parametrize("name", DISTINCT)
def test_reference_signed_sum_is_the_whole_image_gradient(name):
    r = ref.reference(name)
    whole = r["grads"]["means2D"][:, :2]
    scale = max(np.abs(whole).max(), np.abs(r["abs"]).max())
    assert np.abs(r["signed"] - whole).max() <= 1e-12 * scale           # float64: a different summation order only
    assert (r["abs"] >= np.abs(r["signed"]) - 1e-12 * scale).all()      # componentwise
    assert (r["abs"][r["radii"] <= 0] == 0).all()
    assert (r["abs"] > 0).any()


def test_partial_case_has_culled_rows_and_wide_gaussians():
    r = ref.reference("partial")
    assert (r["radii"] <= 0).sum() >= 6                                  # behind the camera / off screen
    P = r["radii"].shape[0]
    tiles = np.zeros(P, int)
    for layer in r["layers"]:
        tiles[layer["ids"].numpy()] += 1
    assert (tiles >= 4).sum() >= 4                                       # several instance slots per Gaussian to sum


def test_cancellation_case_against_its_closed_form():
    r = ref.reference("cancel")
    a, s = ref.cancel_closed_form()
    assert np.abs(r["abs"][0] - a).max() <= 1e-10 * a.max()
    assert np.abs(s).max() <= 1e-12 * a.max() and np.abs(r["signed"][0]).max() <= 1e-12 * a.max()
    # what the feature exists for: the signed norm is nothing, the absolute one is far above the densification threshold
    assert np.linalg.norm(r["abs"][0]) > 100 * 0.0002


def test_long_case_list_and_early_stop():
    r = ref.reference("long")
    tile0 = r["layers"][0]
    n = tile0["ids"].numel()
    assert n > 2 * cases.BATCH2
    contrib = tile0["contrib"].numpy()
    last = np.where(contrib.any(1), contrib.shape[1] - np.argmax(contrib[:, ::-1], 1), 0)      # n_contrib of each pixel
    assert (last < n).sum() > 128                                        # most of its pixels stop before the list ends


@pytest.mark.parametrize("name", cases.NAMES)
def test_fragile_rows_within_the_cap(name):
    rows, visible = ref.fragile_rows(name)
    assert len(rows) <= cases.FRAGILE_ROW_CAP * visible, (rows, visible)


def test_config_switch():
    from luciddreamer_amd import config
    assert config.absgrad() is False
    config.set_absgrad(True)
    try:
        assert config.absgrad() is True
        config.reset()
        assert config.absgrad() is False
        config.set_absgrad(1)
        assert config.absgrad() is True
    finally:
        config.set_absgrad(False)
    assert config.absgrad() is False


def test_exports_and_header():
    from luciddreamer_amd import _lib
    L = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lucid_raster.h")).read()
    assert "lr_view_backward" in _lib.EXPORTS
    getattr(L, "lr_view_backward")
    assert re.search(r"^int\s+lr_view_backward\s*\(const lr_backward_args\*", header, re.M)
    # the statistic is a member of the one backward struct (activated and raw mode alike), right after dL_dmean2D
    m = re.search(r"typedef struct lr_backward_args \{(.*?)\} lr_backward_args;", header, re.S)
    assert m
    members = [x.strip() for x in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";") if x.strip()]
    i = members.index("float* dL_dmean2D")
    assert members[i + 1] == "float* dL_dmean2D_abs"                     # right after dL_dmean2D
    names = [f[0] for f in _lib.BackwardArgs._fields_]
    assert names[names.index("dL_dmean2D") + 1] == "dL_dmean2D_abs"      # ... and in the ctypes mirror
    # a call without it is the call of the other modes: every other member is what they take
    assert [re.split(r"[ *]+", x)[-1] for x in members if x != "float* dL_dmean2D_abs"] == [n for n in names if n != "dL_dmean2D_abs"]


def test_stats_need_the_attribute():
    """With the switch on, add_densification_stats refuses a viewspace tensor without .absgrad instead of using .grad."""
    import torch
    from luciddreamer_amd import config, densify
    vs = torch.zeros(4, 3, requires_grad=True)
    vs.grad = torch.ones(4, 3)
    config.set_absgrad(True)
    try:
        with pytest.raises(RuntimeError, match="absgrad"):
            densify.add_densification_stats(None, vs, torch.ones(4, dtype=torch.int32))
    finally:
        config.set_absgrad(False)
