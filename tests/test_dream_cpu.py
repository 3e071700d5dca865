"""Dreaming without a device: the numpy restatement (tests/dream_ref.py) against what the reference's own host code and scipy make
of two small clouds (tests/golden/ref_dream_fixtures.npz, written by tests/golden/make_dream_fixtures.py), the properties of the
interpolation's definition, the closed-form scale, and the argument checks of the C ABI and of the Python layer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import dream_ref as DR
from tests import reproject_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_dream_fixtures.npz")))


_CASES = {}


def _case(fx, name):
    """The restated frame, correspondences and interpolation of a fixture case, computed once and shared."""
    if name not in _CASES:
        H, W = (int(v) for v in fx[f"{name}_HW"])
        X, C, K, R, T, D = (fx[f"{name}_{k}"] for k in ("X", "C", "K", "R", "T", "depth"))
        fr = RR.project(X, C, K, R, T, H, W)
        corr = DR.border_corr(fr)
        su, sv, sval = DR.correspond(X, fr["pix"], corr, D, K, R, T, H, W, 1.0)
        nd = DR.scatter(su, sv, sval, H, W, fr["mask"])
        _CASES[name] = dict(H=H, W=W, X=X, C=C, K=K, R=R, T=T, D=D, fr=fr, corr=corr, su=su, sv=sv, sval=sval, nd=nd)
    return _CASES[name]


# ---- (b) against the reference's arrays -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_correspondences_against_the_reference(fx, name):
    """The reference forms these lines through torch.matmul and BLAS and with float32 in the middle (inv(R).float(), a float32
    camera origin), the restatement in float64 elementwise: a tolerance, not equality.  Measured on the build container's CPU:
    max |value - compensate_depth| = 7.7e-7 (a) and 7.8e-7 (b) for values up to 1.9; max |uv - pixel_cam2| = 1.4e-14 (a) and
    7.1e-15 (b).  The bars are 4 x the larger of each, the margin for other BLAS builds: 3.2e-6 and 5.7e-14.  The index list is
    the reference's valid_idx[border_valid_idx] exactly, the corners come last and in its order."""
    c = _case(fx, name)
    assert np.array_equal(c["fr"]["mask"], fx[f"{name}_mask2"])
    assert np.array_equal(c["corr"], fx[f"{name}_valid_idx"][fx[f"{name}_border_valid_idx"]])
    M = c["corr"].shape[0]
    uv = np.stack([c["su"], c["sv"]], axis=1)
    assert uv.shape == fx[f"{name}_pixel_cam2"].shape == (M + 4, 2)
    dev_uv = np.abs(uv - fx[f"{name}_pixel_cam2"]).max()
    dev_val = np.abs(c["sval"] - fx[f"{name}_compensate_depth"]).max()
    print(f"{name}: max |uv - pixel_cam2| = {dev_uv:.3g}, max |value - compensate_depth| = {dev_val:.3g}")
    assert np.isfinite(c["sval"]).all()
    assert dev_uv <= 5.7e-14 and dev_val <= 3.2e-6
    assert np.array_equal(uv[M:], [[0, 0], [0, c["H"] - 1], [c["W"] - 1, 0], [c["W"] - 1, c["H"] - 1]])
    assert np.array_equal(c["sval"][M:], np.zeros(4))


@pytest.mark.parametrize("name", ["a", "b"])
def test_difference_from_griddata_is_reported(fx, name, capsys):
    """Reported, not asserted: the interpolation is this library's own definition (DESIGN.md 4b-RPJ has the figures).  What IS
    the reference's: which pixels are appended, in which order, and their colours."""
    c = _case(fx, name)
    hole = fx[f"{name}_hole"]
    assert np.array_equal(hole, np.nonzero(c["fr"]["mask"].reshape(-1) == 0)[0])
    d = np.abs(c["nd"].reshape(-1)[hole].astype(np.float64) - fx[f"{name}_new_depth"])
    pts, cols, info = DR.dream_step(c["X"], c["C"], c["fr"], fx[f"{name}_image"], c["D"], c["K"], c["R"], c["T"], c["H"], c["W"],
                                    "reference")
    N = c["X"].shape[1]
    e = np.abs(pts[:, N:] - fx[f"{name}_new_points"])
    with capsys.disabled():
        print(f"\n{name}: |new_depth - griddata| max {d.max():.4g} median {np.median(d):.4g} (offsets span "
              f"{np.nanmin(c['sval']):.3g} .. {np.nanmax(c['sval']):.3g}); appended points max {e.max():.4g} median "
              f"{np.median(e):.4g}")
    assert info["n_added"] == hole.shape[0] and pts.shape == (3, N + hole.shape[0])
    assert np.array_equal(pts[:, :N], c["X"]) and np.array_equal(cols[:N], c["C"])
    assert np.array_equal(cols[N:], fx[f"{name}_new_colors"])
    assert (c["nd"][c["fr"]["mask"] == 1] == 0).all()


def test_the_reference_fit_never_moves_its_scale(fx):
    """make_dream_fixtures.py runs the reference's 100 Adam steps as written: the scale has no gradient and stays 1."""
    assert fx["a_adam_scale"][0] == 1.0


# ---- (c) the definition's properties ----------------------------------------------------------------------------------------------
H0, W0 = 48, 64
ALL = np.zeros((H0, W0), dtype=np.uint8)


def _samples(seed, n, lo=(4.0, 4.0), hi=(W0 - 5.0, H0 - 5.0)):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), rng


@pytest.mark.parametrize("n", [30, 300])
def test_affine_field_is_reproduced_inside_the_hull(n):
    """An affine field is what the fit is exact for; the corner samples are left out so that nothing disturbs it.  A query is
    inside the hull when it has a sample in each of its four quadrants.  The fit in float64 (_fit64: the restatement's operations
    without the clamp and the rounding) is within 1e-9 of the field (1e-11 measured); the restatement's float32 output adds its
    rounding, half a float32 ulp of values below 8 = 2.4e-7."""
    su, sv, _ = _samples(n, n)
    f = lambda x, y: 2.0 + 0.05 * x - 0.03 * y
    out = DR.scatter(su, sv, f(su, sv), H0, W0, ALL)
    xs, ys = np.meshgrid(np.arange(W0, dtype=np.float64), np.arange(H0, dtype=np.float64), indexing="xy")
    inside = np.zeros((H0, W0), dtype=bool)
    for yy in range(H0):
        for xx in range(W0):
            dx, dy = su - xx, sv - yy
            inside[yy, xx] = all(((sx * dx > 0) & (sy * dy > 0)).any() for sx in (1, -1) for sy in (1, -1))
    assert inside.sum() > 500
    want = f(xs, ys)
    assert np.abs(want).max() < 8
    exact = _fit64(su, sv, f(su, sv), xs[inside], ys[inside])
    print("affine: max |fit - field| =", np.abs(exact - want[inside]).max())
    assert np.abs(exact - want[inside]).max() <= 1e-9
    assert np.abs(out.astype(np.float64) - want)[inside].max() <= 1e-9 + 2.4e-7


def _fit64(su, sv, sval, x, y):
    """The fit of dream_ref.scatter in float64 without the final clamp and rounding (same operations, same order)."""
    S = [np.zeros(x.shape[0]) for _ in range(9)]
    for j in range(len(sval)):
        dx, dy = su[j] - x, sv[j] - y
        d2 = (dx * dx + dy * dy) + 1e-12
        w = 1.0 / (d2 * d2)
        wx, wy, wv = w * dx, w * dy, w * sval[j]
        for k, v in enumerate((w, wx, wy, wx * dx, wx * dy, wy * dy, wv, wv * dx, wv * dy)):
            S[k] = S[k] + v
    S00, S01, S02, S11, S12, S22, B0, B1, B2 = S
    C0, C1, C2 = S11 * S22 - S12 * S12, S02 * S12 - S01 * S22, S01 * S12 - S02 * S11
    return ((B0 * C0 + B1 * C1) + B2 * C2) / ((S00 * C0 + S01 * C1) + S02 * C2)


def test_a_query_on_a_sample_returns_the_sample():
    """On a sample d2 = 1e-12 and w = 1e24; every other sample is at least half a pixel away (w <= 16), so the others weigh
    at most 50 * 16 / 1e24 = 8e-22 of the total and the result is the sample's value up to float64 rounding, far below the float32
    it is rounded to: the float32 of the value, exactly."""
    su, sv, rng = _samples(7, 50)
    su[:5], sv[:5] = [10.0, 20.0, 31.0, 40.0, 55.0], [5.0, 17.0, 30.0, 41.0, 22.0]        # on pixel centres
    far = np.ones(50, dtype=bool)
    for k in range(5):
        d = np.hypot(su - su[k], sv - sv[k])
        far &= (d == 0) | (d >= 0.5)
    assert far.all()
    val = rng.uniform(-2.0, 3.0, 50)
    out = DR.scatter(su, sv, val, H0, W0, ALL)
    for k in range(5):
        assert out[int(sv[k]), int(su[k])] == np.float32(val[k]), k


def test_collinear_samples_take_the_fallback():
    """Samples on one line leave the 3x3 system singular: det is rounding noise (about 1e-16 of S00 S11 S22), below the 1e-12
    threshold at every query, and the result is Shepard's weighted mean B0 / S00, restated here on its own."""
    t = np.linspace(3.0, 60.0, 40)
    su, sv = t, 5.0 + 0.6 * t
    val = np.sin(t / 7.0)
    assert DR.scatter_takes_fallback(su, sv, val, H0, W0, ALL).all()
    out = DR.scatter(su, sv, val, H0, W0, ALL)
    xs, ys = np.meshgrid(np.arange(W0, dtype=np.float64), np.arange(H0, dtype=np.float64), indexing="xy")
    B0, S00 = np.zeros((H0, W0)), np.zeros((H0, W0))
    for j in range(40):
        dx, dy = su[j] - xs, sv[j] - ys
        d2 = (dx * dx + dy * dy) + 1e-12
        w = 1.0 / (d2 * d2)
        S00, B0 = S00 + w, B0 + w * val[j]
    assert np.array_equal(out, (B0 / S00).astype(np.float32))
    # and random samples do not take it
    su, sv, rng = _samples(3, 40)
    assert not DR.scatter_takes_fallback(su, sv, rng.random(40), H0, W0, ALL).any()


def test_no_usable_sample_gives_zero():
    su, sv, rng = _samples(5, 20)
    assert not DR.scatter(su, sv, np.full(20, np.nan), H0, W0, ALL).any()
    assert not DR.scatter(su[:0], sv[:0], np.zeros(0), H0, W0, ALL).any()
    assert not DR.scatter(su, sv, np.zeros(20), H0, W0, ALL).any()                          # samples of 0: exactly 0
    corners = DR.correspond(np.zeros((3, 1), dtype=np.float32), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32),
                            np.ones((H0, W0), dtype=np.float32), np.eye(3), np.eye(3), np.zeros(3), H0, W0)
    assert not DR.scatter(*corners, H0, W0, ALL).any()
    mixed = rng.random(20)
    mixed[::2] = np.nan
    out = DR.scatter(su, sv, mixed, H0, W0, ALL)
    assert np.array_equal(out, DR.scatter(su[1::2], sv[1::2], mixed[1::2], H0, W0, ALL))   # a NaN sample is as if absent


@pytest.mark.parametrize("seed", [1, 2])
def test_no_output_leaves_the_samples_range(seed):
    """A ring of samples around an empty middle and empty outskirts: the unclamped affine fit overshoots there."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, 60)
    su, sv = 32 + 12 * np.cos(ang), 24 + 9 * np.sin(ang)
    val = 0.15 * rng.random(60) * (1 + np.cos(ang))
    out = DR.scatter(su, sv, val, H0, W0, ALL)
    assert out.min() >= np.float32(val.min()) and out.max() <= np.float32(val.max())
    xs, ys = np.meshgrid(np.arange(W0, dtype=np.float64), np.arange(H0, dtype=np.float64), indexing="xy")
    raw = _fit64(su, sv, val, xs.reshape(-1), ys.reshape(-1))
    assert raw.max() > val.max() or raw.min() < val.min()                                   # the clamp does act on this field
    where = (rng.random((H0, W0)) < 0.5).astype(np.uint8)
    part = DR.scatter(su, sv, val, H0, W0, where)
    assert (part[where != 0] == 0).all() and np.array_equal(part[where == 0], out[where == 0])


# ---- (a) the closed-form scale ----------------------------------------------------------------------------------------------------
def test_fit_scale_mathematics():
    """q = P / 1.25 exactly (P a multiple of 1.25 in float64): the scale is 1.25 and the fit cannot be worse than s = 1."""
    from luciddreamer_amd import reproject
    rng = np.random.default_rng(9)
    q = rng.integers(-2000, 2000, (3, 500)).astype(np.float64) / 64.0
    P = q * 1.25
    assert np.array_equal(P / 1.25, q)
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    spp, spq, sqq = (DR._tree_then_sequential(t) for t in (dot(P, P), dot(P, q), dot(q, q)))
    scale, before, after = DR.fit_from_sums(spp, spq, sqq, 500)
    assert abs(scale - 1.25) <= 4 * 2.0 ** -53 * 1.25 * 3 and after <= before and before > 0.01
    assert abs(after) <= 1e-12 * before                                                     # cancellation noise of the three sums only
    fit = reproject.scale_fit_from_sums(spp, spq, sqq, 500)
    assert (fit.scale, fit.n_used, fit.spp, fit.spq, fit.sqq, fit.mse_before, fit.mse_after) == (scale, 500, spp, spq, sqq, before,
                                                                                                 after)
    assert reproject.scale_fit_from_sums(0.0, 0.0, 0.0, 0).scale == 1.0
    assert reproject.scale_fit_from_sums(3.0, 0.0, 0.0, 5).scale == 1.0


def test_scale_sums_drop_non_finite_pairs(fx):
    c = _case(fx, "a")
    D = c["D"].copy()
    pp, pq, qq, use = DR.scale_terms(c["X"], c["fr"]["valid"], c["fr"]["pix"], D, c["K"], c["R"], c["T"], c["H"], c["W"])
    assert use.sum() == c["fr"]["valid"].sum() > 0
    pix = c["fr"]["pix"][np.nonzero(c["fr"]["valid"])[0][[3, 40]]]
    D.reshape(-1)[pix[0]], D.reshape(-1)[pix[1]] = np.nan, np.inf
    lost = int(np.isin(c["fr"]["pix"], pix).sum())
    *_, use2 = DR.scale_terms(c["X"], c["fr"]["valid"], c["fr"]["pix"], D, c["K"], c["R"], c["T"], c["H"], c["W"])
    assert use.sum() - use2.sum() == lost >= 2


# ---- the C ABI on a machine without a device -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


SYMBOLS = ("lr_dream_workspace_bytes", "lr_dream_scale_sums", "lr_dream_correspond", "lr_dream_lift", "lr_scatter_interpolate")


def test_symbols_are_exported_and_built_without_contraction(L):
    from luciddreamer_amd import _lib, build
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert "-ffp-contract=off" in build.SOURCES["dream.hip"]
    assert os.path.exists(os.path.join(build.CSRC, "project_point.h"))
    text = open(os.path.join(build.CSRC, "reproject.hip")).read()
    assert '#include "project_point.h"' in text and "Projected project_point(" not in text    # shared, not copied


def test_workspace_size_is_a_pure_host_function(L):
    w = L.lr_dream_workspace_bytes
    assert w(0) > 0 and w(1) % 256 == 0 and w(1 << 20) >= (1 << 20) // 256 * 32
    assert w(256) <= w(257) <= w(1 << 20) and w(-1) == 0 and w(1 << 31) == 0


@pytest.mark.parametrize("struct, cname", [("DreamArgs", "lr_dream_args"), ("ScatterArgs", "lr_scatter_args")])
def test_ctypes_structures_mirror_the_header(tmp_path, struct, cname):
    from luciddreamer_amd import _lib
    S = getattr(_lib, struct)
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    members = [(f[0], getattr(S, f[0]).offset, getattr(S, f[0]).size) for f in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lucid_raster.h"\nint main(void)\n{\n'
                   f'    printf("sizeof %zu\\n", sizeof({cname}));\n' +
                   "".join(f'    printf("{n} %zu %zu\\n", offsetof({cname}, {n}), sizeof((({cname}*)0)->{n}));\n'
                           for n, _, _ in members) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(S)}"
    assert lines[1:1 + len(members)] == [f"{n} {o} {s}" for n, o, s in members]
    end = 0
    for n, o, s in members:
        assert 0 <= o - end < 8, n
        end = o + s
    assert 0 <= ctypes.sizeof(S) - end < 8
    assert _lib.LR_SCATTER_TILE == 256 and "#define LR_SCATTER_TILE 256" in open(os.path.join(ROOT, "include", "lucid_raster.h")).read()


_BUF = (ctypes.c_double * 72)()
PTR = (ctypes.addressof(_BUF) + 15) & ~15               # non-NULL, 16-byte aligned, never dereferenced by the checks
_EYE = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
_ZERO = (ctypes.c_double * 3)(0, 0, 0)
_NAN9 = (ctypes.c_double * 9)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1)


def _dream_args(**fields):
    from luciddreamer_amd import _lib
    eye, zero = ctypes.addressof(_EYE), ctypes.addressof(_ZERO)
    a = dict(n_points=100, points=PTR, point_stride=3, coord_stride=1, valid=PTR, pix=PTR, height=48, width=64, depth=PTR,
             K=eye, R=eye, T=zero, Kinv=eye, Rinv=eye, RinvT=zero, scale=1.0, corr=PTR, n_corr=10, out_su=PTR, out_sv=PTR,
             out_sval=PTR, out_sums=PTR, out_count=PTR, new_depth=PTR, out_points=PTR, workspace=PTR, workspace_bytes=1 << 20)
    a.update(fields)
    return _lib.DreamArgs(**a)


NAN9 = ctypes.addressof(_NAN9)
DREAM_REJECTED = {
    "sums_negative_n": ("lr_dream_scale_sums", dict(n_points=-1), b"n_points"),
    "sums_height_0": ("lr_dream_scale_sums", dict(height=0), b"height, width"),
    "sums_pixels_beyond_int": ("lr_dream_scale_sums", dict(height=65536, width=65536), b"H*W"),
    "sums_no_depth": ("lr_dream_scale_sums", dict(depth=None), b"depth"),
    "sums_no_Kinv": ("lr_dream_scale_sums", dict(Kinv=None), b"Kinv, Rinv and RinvT are required"),
    "sums_nan_Rinv": ("lr_dream_scale_sums", dict(Rinv=NAN9), b"finite"),
    "sums_no_points": ("lr_dream_scale_sums", dict(points=None), b"points and pix"),
    "sums_no_pix": ("lr_dream_scale_sums", dict(pix=None), b"points and pix"),
    "sums_no_valid": ("lr_dream_scale_sums", dict(valid=None), b"valid"),
    "sums_zero_stride": ("lr_dream_scale_sums", dict(coord_stride=0), b"stride"),
    "sums_no_out": ("lr_dream_scale_sums", dict(out_sums=None), b"out_sums"),
    "sums_misaligned_count": ("lr_dream_scale_sums", dict(out_count=PTR + 4), b"out_sums"),
    "sums_no_workspace": ("lr_dream_scale_sums", dict(workspace=None), b"workspace"),
    "sums_small_workspace": ("lr_dream_scale_sums", dict(n_points=1 << 20, workspace_bytes=(1 << 17) - 1), b"workspace"),
    "corr_negative_m": ("lr_dream_correspond", dict(n_corr=-1), b"n_corr"),
    "corr_m_beyond_int": ("lr_dream_correspond", dict(n_corr=(1 << 31) - 4), b"n_corr"),
    "corr_no_list": ("lr_dream_correspond", dict(corr=None), b"corr is required"),
    "corr_no_K": ("lr_dream_correspond", dict(K=None), b"K, R and T are required"),
    "corr_nan_R": ("lr_dream_correspond", dict(R=NAN9), b"finite"),
    "corr_nan_scale": ("lr_dream_correspond", dict(scale=float("nan")), b"scale"),
    "corr_no_out": ("lr_dream_correspond", dict(out_sv=None), b"out_su"),
    "corr_misaligned_out": ("lr_dream_correspond", dict(out_sval=PTR + 4), b"out_su"),
    "lift_no_new_depth": ("lr_dream_lift", dict(new_depth=None), b"new_depth"),
    "lift_no_out": ("lr_dream_lift", dict(out_points=None), b"new_depth and out_points"),
    "lift_inf_scale": ("lr_dream_lift", dict(scale=float("inf")), b"scale"),
    "lift_width_0": ("lr_dream_lift", dict(width=0), b"height, width"),
}


@pytest.mark.parametrize("case", sorted(DREAM_REJECTED))
def test_dream_entry_points_reject_without_a_device(L, case):
    from luciddreamer_amd import _lib
    fn, fields, message = DREAM_REJECTED[case]
    assert getattr(L, fn)(_dream_args(**fields)) == _lib.LR_ERR_INVALID_ARG
    assert message in L.lr_last_error() and fn.encode() in L.lr_last_error(), L.lr_last_error()


def _scatter_args(**fields):
    from luciddreamer_amd import _lib
    a = dict(n_samples=10, su=PTR, sv=PTR, sval=PTR, height=48, width=64, where=PTR, out=PTR)
    a.update(fields)
    return _lib.ScatterArgs(**a)


SCATTER_REJECTED = {
    "negative_m": (dict(n_samples=-1), b"n_samples"),
    "m_beyond_int": (dict(n_samples=1 << 31), b"n_samples"),
    "no_su": (dict(su=None), b"su, sv and sval are required"),
    "no_sval": (dict(sval=None), b"su, sv and sval are required"),
    "misaligned_sv": (dict(sv=PTR + 4), b"8-byte"),
    "height_0": (dict(height=0), b"height, width"),
    "pixels_beyond_int": (dict(height=65536, width=65536), b"H*W"),
    "no_where": (dict(where=None), b"where and out"),
    "no_out": (dict(out=None), b"where and out"),
    "misaligned_out": (dict(out=PTR + 2), b"4-byte"),
}


@pytest.mark.parametrize("case", sorted(SCATTER_REJECTED))
def test_scatter_interpolate_rejects_without_a_device(L, case):
    from luciddreamer_amd import _lib
    fields, message = SCATTER_REJECTED[case]
    assert L.lr_scatter_interpolate(_scatter_args(**fields)) == _lib.LR_ERR_INVALID_ARG
    assert message in L.lr_last_error(), L.lr_last_error()


def test_struct_bytes_is_checked_first(L):
    from luciddreamer_amd import _lib
    for fn in (L.lr_dream_scale_sums, L.lr_dream_correspond, L.lr_dream_lift):
        assert fn(None) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
        a = _dream_args(n_points=-1, height=0, depth=None, Kinv=None)     # everything else is wrong as well
        a.struct_bytes -= 8
        assert fn(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    assert L.lr_scatter_interpolate(None) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    s = _scatter_args(n_samples=-1, where=None)
    s.struct_bytes += 8
    assert L.lr_scatter_interpolate(s) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()


# ---- the public interface ----------------------------------------------------------------------------------------------------
def test_package_exports_the_new_names():
    import luciddreamer_amd
    r = luciddreamer_amd.reproject
    for name in ("fit_scale", "scatter_interpolate", "compensate", "dream_step", "ScaleFit", "Compensation", "DreamInfo"):
        assert hasattr(r, name), name
    assert r.ScaleFit._fields == ("scale", "n_used", "spp", "spq", "sqq", "mse_before", "mse_after")
    assert r.Compensation._fields == ("new_depth", "lifted", "n_corr", "corr_uv", "corr_value")
    assert luciddreamer_amd.dream_step is r.dream_step and luciddreamer_amd.fit_scale is r.fit_scale
    assert r.SCATTER_TILE == DR.BLOCK == 256


def _host_frame(H, W, N, batched=False):
    from luciddreamer_amd import reproject
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    lead = (2,) if batched else ()
    return reproject.Frame(torch.zeros(*lead, H, W, 3), u8(*lead, H, W), u8(*lead, H, W), u8(*lead, H, W), torch.zeros(*lead, H, W),
                           None if batched else u8(N), None if batched else torch.zeros(N, dtype=torch.int32), u8(*lead, H, W, 3))


def test_host_tensors_and_batched_frames_raise():
    from luciddreamer_amd import reproject
    H, W, N = 8, 8, 10
    X, C, D, img = torch.rand(3, N), torch.rand(N, 3), torch.rand(H, W), torch.zeros(H, W, 3, dtype=torch.uint8)
    K, R, T = np.eye(3), np.eye(3), np.zeros((3, 1))
    one, many = _host_frame(H, W, N), _host_frame(H, W, N, batched=True)
    for call in (lambda f: reproject.fit_scale(X, f, D, K, R, T),
                 lambda f: reproject.compensate(X, f, D, K, R, T),
                 lambda f: reproject.dream_step(X, C, f, img, D, K, R, T)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call(one)
        with pytest.raises(ValueError, match="one pose"):
            call(many)
        with pytest.raises(TypeError, match="Frame"):
            call((1, 2, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        reproject.scatter_interpolate(torch.zeros(3, 2, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), H, W,
                                      torch.zeros(H, W, dtype=torch.uint8))
