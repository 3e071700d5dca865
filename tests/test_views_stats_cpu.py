"""CPU: densification statistics inside the multi-view step (lr_views_args stat_* members, ViewBatch(densify_stats=...)).
The argument rules of the C call and of ViewBatch, which sit in front of any device work, and the statistics the float64
per-pixel reference (tests/absgrad_ref.py) gives for the cases tests/test_gpu_views_stats.py runs on the GPU."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import absgrad_cases as cases
from tests import absgrad_ref as ref

STAT_CASES = ("partial", "cancel", "long", "partial_depth_alpha", "partial_aa")
STAT_MEMBERS = ("stat_grad_accum", "stat_denom", "stat_max_radii")
THRESHOLD = 0.0002                      # the reference's densify_grad_threshold


@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


def reference_stats(name):
    """(signed norm, absolute norm, visible) per Gaussian of one view of the case, float64: what one view adds to
    xyz_gradient_accum in "grad" / "absgrad" mode, and the rows it adds 1 to denom for."""
    r = ref.reference(name)
    vis = r["radii"] > 0
    signed = np.where(vis, np.linalg.norm(r["grads"]["means2D"][:, :2], axis=1), 0.0)
    absolute = np.where(vis, np.linalg.norm(r["abs"], axis=1), 0.0)
    return signed, absolute, vis


# ---- the C call ----------------------------------------------------------------------------------------------------------------
def _args(given, absgrad=0):
    from luciddreamer_amd import _lib
    buf = (ctypes.c_float * 16)()
    a = _lib.ViewsArgs(n_views=2, P=0, stat_absgrad=absgrad, **{m: ctypes.addressof(buf) for m in given})
    a._keep = buf
    return a


PARTIAL = [c for k in (1, 2) for c in itertools.combinations(STAT_MEMBERS, k)]


@pytest.mark.parametrize("given", PARTIAL, ids=["+".join(m[5:] for m in c) for c in PARTIAL])
def test_partial_stat_pointers_are_rejected(L, given):
    from luciddreamer_amd import _lib
    assert len(PARTIAL) == 6
    assert L.lr_views_accumulate(_args(given)) == _lib.LR_ERR_INVALID_ARG
    msg = L.lr_last_error()
    assert all(m.encode() in msg for m in STAT_MEMBERS), msg


def test_stat_absgrad_without_pointers_is_rejected(L):
    from luciddreamer_amd import _lib
    assert L.lr_views_accumulate(_args((), absgrad=1)) == _lib.LR_ERR_INVALID_ARG
    msg = L.lr_last_error()
    assert b"stat_absgrad" in msg and all(m.encode() in msg for m in STAT_MEMBERS), msg


def test_all_or_none_with_nothing_to_do_returns_zero(L):
    assert L.lr_views_accumulate(_args(())) == 0
    assert L.lr_views_accumulate(_args(STAT_MEMBERS)) == 0
    assert L.lr_views_accumulate(_args(STAT_MEMBERS, absgrad=1)) == 0


def test_version_and_mirror(L):
    from luciddreamer_amd import _lib
    assert b" 0.6.3" in L.lr_version()
    names = [f[0] for f in _lib.ViewsArgs._fields_]
    i = names.index("acc_rot")
    assert names[i + 1:i + 5] == list(STAT_MEMBERS) + ["stat_absgrad"]


# ---- ViewBatch -----------------------------------------------------------------------------------------------------------------
def _batch(**kw):
    from luciddreamer_amd import cameras, parallel
    cam = cameras.identity_camera(16, 16)
    return parallel.ViewBatch([cam], [torch.zeros(3, 16, 16)], 0, torch.zeros(3), binning_capacity=1024, **kw)


def _cloud(P=8):
    z = torch.zeros
    return (z(P, 3), z(P, 1), z(P, 3), z(P, 4), z(P, 1, 3)), {"means3D": z(P, 3), "means2D": z(P, 3), "opacity": z(P, 1),
                                                                "sh": z(P, 1, 3), "scales": z(P, 3), "rotations": z(P, 4)}


def _stats(P=8, **over):
    s = {"xyz_gradient_accum": torch.zeros(P, 1), "denom": torch.zeros(P, 1), "max_radii2D": torch.zeros(P)}
    s.update(over)
    return s


def test_view_batch_rejects_an_unknown_mode():
    with pytest.raises(ValueError, match="densify_stats"):
        _batch(densify_stats="abs")


def test_view_batch_stats_and_mode_go_together(L):
    params, acc = _cloud()
    with pytest.raises(ValueError, match="densify_stats"):
        _batch().run(*params, acc, stats=_stats())
    for mode in ("grad", "absgrad"):
        with pytest.raises(ValueError, match="stats"):
            _batch(densify_stats=mode).run(*params, acc)


@pytest.mark.parametrize("bad", [
    dict(denom=torch.zeros(7, 1)), dict(max_radii2D=torch.zeros(8, 2)), dict(xyz_gradient_accum=torch.zeros(8, 1, dtype=torch.float64)),
    dict(denom=torch.zeros(8, 2)[:, :1]), dict(max_radii2D=torch.zeros(8, dtype=torch.int32)), dict(denom=None),
    dict(extra=torch.zeros(8))], ids=["rows", "columns", "float64", "strided", "int32", "none", "extra_key"])
def test_view_batch_rejects_wrong_stats(L, bad):
    params, acc = _cloud()
    with pytest.raises(ValueError, match="stats"):
        _batch(densify_stats="grad").run(*params, acc, stats=_stats(**bad))
    missing = _stats()
    del missing["denom"]
    with pytest.raises(ValueError, match="stats"):
        _batch(densify_stats="grad").run(*params, acc, stats=missing)


def test_view_batch_rejects_host_stats_before_any_device_work(L):
    params, acc = _cloud()
    with pytest.raises(ValueError, match="HIP device"):
        _batch(densify_stats="absgrad").run(*params, acc, stats=_stats())


# ---- the reference statistics --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STAT_CASES)
def test_reference_statistics(name):
    signed, absolute, vis = reference_stats(name)
    rows, visible = ref.fragile_rows(name)
    assert visible == int(vis.sum()) > 0
    assert len(rows) <= cases.FRAGILE_ROW_CAP * visible                  # the GPU test may leave these rows out
    assert np.isfinite(signed).all() and np.isfinite(absolute).all()
    assert not signed[~vis].any() and not absolute[~vis].any()
    # |sum| <= sum |.| componentwise, hence for the norms
    assert (signed <= absolute * (1 + 1e-12) + 1e-300).all()
    assert absolute.max() > 0                                            # (a fully occluded Gaussian has none: case "long")


def test_cancel_case_separates_the_two_statistics():
    """What tests/test_gpu_views_stats.py's densify-rule test stands on: at the reference's threshold the signed statistic
    does not select the broad Gaussian and the absolute one does."""
    signed, absolute, vis = reference_stats("cancel")
    assert vis.tolist() == [True]
    assert signed[0] < THRESHOLD < absolute[0]
