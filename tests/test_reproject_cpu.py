"""Point-cloud reprojection without a device: the numpy restatement (tests/reproject_ref.py) against what the reference's own
host code and scipy make of the fixture clouds (tests/golden/ref_reproject_fixtures.npz, written by
tests/golden/make_reproject_fixtures.py), and the C ABI's argument checks."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import reproject_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_reproject_fixtures.npz")))


_FRAMES = {}


def _frame(fx, name, colors=None):
    key = (name, colors is not None)
    if key not in _FRAMES:
        H, W = (int(v) for v in fx[f"{name}_HW"])
        C = fx[f"{name}_C"] if colors is None else colors
        _FRAMES[key] = RR.project(fx[f"{name}_X"], C, fx[f"{name}_K"], fx[f"{name}_R"], fx[f"{name}_T"], H, W)
    return _FRAMES[key]


# ---- the restatement against the reference's arrays: exact, no point left out --------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "grid"])
def test_masks_and_indices_equal_the_reference(fx, name):
    """The reference forms R X + T through BLAS, the restatement elementwise: a point could be left out of the comparison only
    if it sat within 1e-9 of a rounding tie or a bound (the generator asserts none does).  The cap on left-out points is 0."""
    H, W = (int(v) for v in fx[f"{name}_HW"])
    r = _frame(fx, name)
    valid_idx = np.nonzero(r["valid"])[0]
    assert np.array_equal(valid_idx, fx[f"{name}_valid_idx"])
    pix = r["pix"][valid_idx]
    assert np.array_equal(np.stack([pix % W, pix // W]), fx[f"{name}_round_coord"])
    assert (r["pix"][r["valid"] == 0] == -1).all()
    assert np.array_equal(r["hit"], fx[f"{name}_hit"])
    assert np.array_equal(r["dil"], fx[f"{name}_round_mask"])
    assert np.array_equal(r["mask"], fx[f"{name}_mask2"])
    assert np.array_equal(r["border"], fx[f"{name}_mask_hf"])
    border_valid_idx = np.nonzero(r["border"].reshape(-1)[pix])[0]
    assert np.array_equal(border_valid_idx, fx[f"{name}_border_valid_idx"])


def test_fixture_clouds_have_holes_borders_and_rejected_points(fx):
    for name in ("a", "b"):
        H, W = (int(v) for v in fx[f"{name}_HW"])
        m = fx[f"{name}_mask2"]
        assert 0 < m.sum() < H * W and fx[f"{name}_mask_hf"].any()
        assert 0 < fx[f"{name}_valid_idx"].size < fx[f"{name}_X"].shape[1]
        assert (fx[f"{name}_round_mask"] >= m).all() and (fx[f"{name}_round_mask"] >= fx[f"{name}_hit"]).all()


# ---- the two bounds against griddata that can be derived -----------------------------------------------------------------------
def test_lifted_grid_at_its_own_pose_matches_griddata(fx):
    """Every u, v is integral: one neighbour takes the whole weight, the image is the point's colour in 16-bit fixed point.
    Bound: the colour step 0.5 / 65535 = 7.6e-6 plus float32 rounding (6e-8) < 1e-5."""
    r = _frame(fx, "grid")
    assert r["mask"].all() and np.array_equal(RR.lift(fx["grid_depth"], fx["grid_K"], fx["grid_R"], fx["grid_T"]), fx["grid_X"])
    err = np.abs(r["image"].astype(np.float64) - fx["grid_griddata"])[r["mask"] == 1]
    print("lifted grid: max |image - griddata| =", err.max())
    assert err.max() <= 1e-5
    assert np.array_equal(r["depth"], fx["grid_depth"])


def test_constant_colour_cloud_gives_the_constant(fx):
    """Every weighted mean of one colour is that colour: within the 16-bit colour step plus float32 rounding, < 1e-5, wherever
    griddata interpolated (it writes its fill value 0 outside the hull of the projected points)."""
    const = fx["b_const_color"]
    N = fx["b_X"].shape[1]
    r = _frame(fx, "b", colors=np.tile(const, (N, 1)))
    g = fx["b_const_griddata"]
    inside = (r["mask"] == 1) & (g != 0).all(-1)
    assert inside.sum() > 100
    err = np.abs(r["image"].astype(np.float64) - g)[inside]
    print("constant colour: max |image - griddata| =", err.max())
    assert err.max() <= 1e-5
    assert (np.abs(r["image"][r["mask"] == 1].astype(np.float64) - const.astype(np.float64)) <= 1e-5).all()
    assert (r["image"][r["mask"] == 0] == 0).all()


def test_restatement_invariants(fx):
    r = _frame(fx, "a")
    assert (r["S"][r["hit"] == 1] >= 16384).all()                 # what the window fill relies on
    assert (r["image"][r["mask"] == 0] == 0).all() and (r["depth"][r["mask"] == 0] == 0).all()
    assert np.isfinite(r["image"]).all() and r["image"].max() <= 1.0
    occluded = RR.project(fx["a_X"], fx["a_C"], fx["a_K"], fx["a_R"], fx["a_T"], 48, 64, z_tolerance=1e9)
    assert not np.array_equal(occluded["image"], r["image"])      # the z test rejects the far layer behind the near one
    assert np.array_equal(occluded["mask"], r["mask"])


def test_pc2w_equals_the_restated_formula():
    from luciddreamer_amd import reproject
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q2, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Tw2i, Ti2j = rng.normal(size=(3, 1)), rng.normal(size=(3, 1))
    Rw2j, Tw2j = reproject.compose_pose(q2, Ti2j, q, Tw2i)
    assert np.array_equal(Rw2j, q2 @ q) and np.array_equal(Tw2j, q2 @ Tw2i + Ti2j)
    P = reproject.pc2w(Rw2j, Tw2j)
    flip = np.diag([1.0, -1.0, -1.0])
    want = np.eye(4)
    want[:3, :3] = (flip @ Rw2j).T
    want[:3, 3:] = -(flip @ Rw2j).T @ (flip @ Tw2j)
    assert P.shape == (4, 4) and np.array_equal(P, want) and np.array_equal(P, RR.pc2w(Rw2j, Tw2j))
    # camera to world: the camera centre -inv(R) T, the axes those of the world-to-camera rotation with y and z reversed
    assert np.allclose(P[:3, 3:], -np.linalg.inv(Rw2j) @ Tw2j, atol=1e-12)
    assert np.allclose(P[:3, :3] @ (flip @ Rw2j), np.eye(3), atol=1e-12)


# ---- the C ABI on a machine without a device -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


SYMBOLS = ("lr_reproject_workspace_bytes", "lr_reproject", "lr_lift")


def test_symbols_are_exported(L):
    from luciddreamer_amd import _lib
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert "reproject.hip" in __import__("luciddreamer_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "-ffp-contract=off" in __import__("luciddreamer_amd.build", fromlist=["SOURCES"]).SOURCES["reproject.hip"]


def test_workspace_size_is_a_pure_host_function(L):
    w = L.lr_reproject_workspace_bytes
    assert w(1, 48, 64) > 0 and w(1, 48, 64) % 256 == 0 and w(5, 37, 53) % 256 == 0
    assert w(1, 48, 64) < w(2, 48, 64) < w(5, 48, 64) < w(5, 512, 512)
    assert w(1, 48, 64) < w(1, 49, 64) < w(1, 49, 65)
    assert w(1, 512, 512) >= 512 * 512 * (32 + 4 + 1 + 1)            # the accumulators, zmin, dilated, mask
    assert w(0, 48, 64) == 0 and w(1, 1, 64) == 0 and w(1, 65536, 65536) == 0 and w(65536, 48, 64) == 0


def test_ctypes_structure_mirrors_the_header(tmp_path):
    from luciddreamer_amd import _lib
    S = _lib.ReprojectArgs
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    members = [(f[0], getattr(S, f[0]).offset, getattr(S, f[0]).size) for f in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lucid_raster.h"\nint main(void)\n{\n'
                   '    printf("sizeof %zu\\n", sizeof(lr_reproject_args));\n' +
                   "".join(f'    printf("{n} %zu %zu\\n", offsetof(lr_reproject_args, {n}), '
                           f'sizeof(((lr_reproject_args*)0)->{n}));\n' for n, _, _ in members) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(S)}"
    assert lines[1:1 + len(members)] == [f"{n} {o} {s}" for n, o, s in members]
    end = 0
    for n, o, s in members:                      # every member of the C struct is mirrored: no gap beyond alignment padding
        assert 0 <= o - end < 8, n
        end = o + s
    assert 0 <= ctypes.sizeof(S) - end < 8


_BUF = (ctypes.c_double * 72)()
PTR = (ctypes.addressof(_BUF) + 15) & ~15               # non-NULL, 16-byte aligned, never dereferenced by the checks
_EYE = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
_ZERO = (ctypes.c_double * 3)(0, 0, 0)


def _mat(values):
    return (ctypes.c_double * len(values))(*values)


def _args(**fields):
    from luciddreamer_amd import _lib
    a = dict(n_points=100, points=PTR, point_stride=3, coord_stride=1, colors=PTR, n_frames=1, height=48, width=64,
             z_tolerance=0.05, K=ctypes.addressof(_EYE), R=ctypes.addressof(_EYE), T=ctypes.addressof(_ZERO),
             out_image=PTR, out_mask=PTR, out_valid=PTR, out_pix=PTR, workspace=PTR, workspace_bytes=1 << 30)
    a.update(fields)
    keep = [v for v in a.values() if isinstance(v, ctypes.Array)]
    a = {k: (ctypes.addressof(v) if isinstance(v, ctypes.Array) else v) for k, v in a.items()}
    s = _lib.ReprojectArgs(**a)
    s._keep = keep
    return s


REJECTED = {
    "negative_n": (dict(n_points=-1), b"n_points"),
    "n_beyond_int": (dict(n_points=1 << 31), b"n_points"),
    "no_frames": (dict(n_frames=0), b"n_frames"),
    "too_many_frames": (dict(n_frames=65536), b"n_frames"),
    "height_1": (dict(height=1), b"height and width"),
    "pixels_beyond_int": (dict(height=65536, width=65536), b"H*W"),
    "no_K": (dict(K=None), b"K, R and T are required"),
    "no_R": (dict(R=None), b"K, R and T are required"),
    "no_T": (dict(T=None), b"K, R and T are required"),
    "nan_K": (dict(K=_mat([1, 0, 0, 0, float("nan"), 0, 0, 0, 1])), b"finite"),
    "inf_R": (dict(R=_mat([1, 0, 0, 0, 1, 0, 0, float("inf"), 1])), b"finite"),
    "nan_T": (dict(T=_mat([0, float("nan"), 0])), b"finite"),
    "nan_tolerance": (dict(z_tolerance=float("nan")), b"z_tolerance"),
    "inf_tolerance": (dict(z_tolerance=float("inf")), b"z_tolerance"),
    "negative_tolerance": (dict(z_tolerance=-0.01), b"z_tolerance"),
    "no_points": (dict(points=None), b"points are required"),
    "no_colors_with_image": (dict(colors=None), b"colors"),
    "no_colors_with_u8": (dict(colors=None, out_image=None, out_image_u8=PTR), b"colors"),
    "zero_stride": (dict(point_stride=0), b"stride"),
    "valid_with_frames": (dict(n_frames=2, R=_mat([1, 0, 0, 0, 1, 0, 0, 0, 1] * 2), T=_mat([0] * 6), out_pix=None), b"n_frames == 1"),
    "pix_with_frames": (dict(n_frames=2, R=_mat([1, 0, 0, 0, 1, 0, 0, 0, 1] * 2), T=_mat([0] * 6), out_valid=None), b"n_frames == 1"),
    "no_workspace": (dict(workspace=None), b"workspace"),
    "misaligned_workspace": (dict(workspace=PTR + 4), b"workspace"),
    "small_workspace": (dict(workspace_bytes=48 * 64 * 38 - 1), b"workspace"),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_reproject_rejects_without_a_device(L, case):
    from luciddreamer_amd import _lib
    fields, message = REJECTED[case]
    assert L.lr_reproject(_args(**fields)) == _lib.LR_ERR_INVALID_ARG
    assert message in L.lr_last_error(), L.lr_last_error()


def test_reproject_checks_struct_bytes_first(L):
    from luciddreamer_amd import _lib
    assert L.lr_reproject(None) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    a = _args(n_points=-1, K=None, workspace=None)                # everything else is wrong as well
    a.struct_bytes -= 8
    assert L.lr_reproject(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()


def test_lift_rejects_without_a_device(L):
    from luciddreamer_amd import _lib
    eye, zero = ctypes.addressof(_EYE), ctypes.addressof(_ZERO)
    bad = _mat([1, 0, 0, 0, float("nan"), 0, 0, 0, 1])
    bad3 = _mat([0, 0, float("inf")])
    for args, message in (((0, 64, PTR, eye, eye, zero, PTR, None), b"positive"),
                          ((65536, 65536, PTR, eye, eye, zero, PTR, None), b"H*W"),
                          ((48, 64, None, eye, eye, zero, PTR, None), b"required"),
                          ((48, 64, PTR, None, eye, zero, PTR, None), b"required"),
                          ((48, 64, PTR, eye, None, zero, PTR, None), b"required"),
                          ((48, 64, PTR, eye, eye, None, PTR, None), b"required"),
                          ((48, 64, PTR, eye, eye, zero, None, None), b"required"),
                          ((48, 64, PTR, ctypes.addressof(bad), eye, zero, PTR, None), b"finite"),
                          ((48, 64, PTR, eye, ctypes.addressof(bad), zero, PTR, None), b"finite"),
                          ((48, 64, PTR, eye, eye, ctypes.addressof(bad3), PTR, None), b"finite")):
        assert L.lr_lift(*args) == _lib.LR_ERR_INVALID_ARG
        assert message in L.lr_last_error(), (args, L.lr_last_error())


# ---- the public interface ----------------------------------------------------------------------------------------------------
def test_package_exports_the_module():
    import luciddreamer_amd
    r = luciddreamer_amd.reproject
    for name in ("lift", "project", "project_batch", "align_frames", "compose_pose", "pc2w", "Frame"):
        assert hasattr(r, name), name
    assert r.Frame._fields[:7] == ("image", "mask", "dilated", "border", "depth", "valid", "pix")


def test_host_tensors_raise():
    from luciddreamer_amd import reproject
    X, C = torch.rand(10, 3), torch.rand(10, 3)
    K, R, T = np.eye(3), np.eye(3), np.zeros((3, 1))
    poses = np.tile(np.eye(4)[None], (2, 1, 1))
    for call in (lambda: reproject.project(X, C, K, R, T, 8, 8),
                 lambda: reproject.project_batch(X, C, K, np.stack([R, R]), np.stack([T, T]), 8, 8),
                 lambda: reproject.lift(torch.rand(8, 8), K, R, T),
                 lambda: reproject.align_frames(X, C, K, poses, poses, 8, 8, 1.0)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
