"""TSDF fusion and mesh extraction without a device: the numpy restatement (tests/tsdf_ref.py) is sound -- fusing a plane gives
the distance to it, the meshes of analytic fields are closed, oriented and have the right genus --, pinhole_of agrees with the
rasterizer's projection, and the C ABI refuses every bad argument in front of its first HIP call."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import posed_cases
from tests import tsdf_cases as TC
from tests import tsdf_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement: integration ------------------------------------------------------------------------------------------------
def test_fronto_parallel_plane_gives_the_distance():
    """A camera at the origin looking down +z at the plane z = d0: every touched voxel holds (d0 - z) / trunc clamped at 1,
    within 2 float32 ulp; voxels more than trunc behind the plane stay untouched."""
    d0, trunc, H, W = 2.0, 0.3, 40, 40
    K = np.array([[30.0, 0.0, 19.5], [0.0, 30.0, 19.5], [0.0, 0.0, 1.0]])
    vol = TR.RefVolume((-0.45, -0.45, 1.25), 0.1, (10, 10, 14), trunc)
    touched = vol.integrate(np.full((1, H, W), d0, dtype=np.float32), K, np.eye(3)[None], np.zeros((1, 3)))
    z = vol.axis_coords(2).astype(np.float64)[:, None, None] * np.ones(vol.tsdf.shape)
    behind = z > d0 + trunc + 1e-6
    assert touched.any() and behind.any() and (z < d0 - trunc).any()
    assert not touched[behind].any()
    assert np.array_equal(touched, ~behind)                      # the whole volume is inside the frustum
    assert np.array_equal(vol.tsdf[~touched], np.ones(int((~touched).sum()), dtype=np.float32))
    assert np.array_equal(vol.weight, touched.astype(np.float32))
    want = np.minimum(1.0, (d0 - z) / trunc)
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(2.0 ** -126)).astype(np.float32)).astype(np.float64)
    # z is the float32 lattice coordinate on both sides (K's last row is (0,0,1), R = I, T = 0) and d0 - z is exact
    err = np.abs(vol.tsdf.astype(np.float64) - want)[touched]
    bound = (2 * ulp)[touched]
    print(f"plane: max err / ulp {(err / ulp[touched]).max():.3f}")
    assert (err <= bound).all()


def test_frames_one_at_a_time_equal_the_batch_in_the_restatement():
    a = TC.integrate_inputs()
    whole, _ = TC.integrate_reference("weights")
    vol = TC.new_int_volume()
    for f in range(TC.INT_F):
        vol.integrate(a["depths"][f:f + 1], a["K"], a["Rs"][f:f + 1], a["Ts"][f:f + 1], colors=a["colors"][f:f + 1],
                      pixel_weights=a["pixel_weights"][f:f + 1])
    for name in ("tsdf", "weight", "color"):
        assert np.array_equal(getattr(vol, name), getattr(whole, name)), name


def test_integration_case_is_fit_for_its_comparison():
    """The GPU case reaches what it aims at: touched and untouched voxels, a frame that sees nothing, rejected pixels of every
    kind under projected voxels, clamped weights and a depth limit that bites."""
    a = TC.integrate_inputs()
    plain, touched = TC.integrate_reference("plain")
    assert 0 < touched.sum() < touched.size
    behind = TC.new_int_volume()
    assert not behind.integrate(a["depths"][3:4], a["K"], a["Rs"][3:4], a["Ts"][3:4]).any()      # the volume behind the camera
    assert np.array_equal(plain.color, np.zeros_like(plain.color))                                 # colour untouched without a stack
    for bad in (0.0, np.nan, np.inf, -1.5):
        hit = np.isnan(a["depths"]) if bad != bad else a["depths"] == np.float32(bad)
        assert hit.any(axis=(1, 2)).all()
    limits, t2 = TC.integrate_reference("limits")
    assert 0 < t2.sum() < touched.sum() and limits.weight.max() == np.float32(2.5)
    weights, t3 = TC.integrate_reference("weights")
    assert t3.sum() < touched.sum()
    assert (plain.tsdf[touched] < 0).any() and (plain.tsdf[touched] == 1).any()


# ---- the restatement: extraction -----------------------------------------------------------------------------------------------------
def test_winding_table_is_combinatorially_complete():
    for t in range(6):
        assert TR.TRIANGLES[t][0] == () and TR.TRIANGLES[t][15] == ()
        for m in range(1, 15):
            n_in = bin(m).count("1")
            tris = TR.TRIANGLES[t][m]
            assert len(tris) == (2 if n_in == 2 else 1)
            for tri in tris:                                       # every edge joins an inside and an outside vertex
                assert all(((m >> lo) & 1) != ((m >> hi) & 1) and lo < hi for lo, hi in tri)
            # the complement mask gives the same triangle with the opposite winding (a quad: the same four edges)
            other = TR.TRIANGLES[t][15 - m]
            if n_in != 2:
                assert ((tris[0][0], tris[0][2], tris[0][1]),) == other
            assert {e for tri in tris for e in tri} == {e for tri in other for e in tri}


def test_sphere_mesh_is_a_closed_oriented_sphere():
    V, C, F = TC.field_mesh("sphere")
    assert TR.is_closed(F) and TR.euler(len(V), F) == 2 and TR.all_referenced(len(V), F)
    tri = V[F].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((n * (tri.mean(axis=1) - TC.SPHERE_C)).sum(axis=1) > 0).all()         # every triangle faces away from the centre
    # an edge of length <= L = sqrt(3) s that crosses the sphere stays within L of it, so at distance >= r - L from the centre;
    # along it the distance function is convex with second derivative <= 1 / (r - L), and a chord of a function with second
    # derivative <= k over a length L leaves it by at most k L^2 / 8.  The interpolated root is that close to the sphere
    # (the field is not clamped there: |f| <= L < trunc).  1e-5: float32 positions of size 20.
    L = math.sqrt(3.0) * TC.FIELD_S
    bound = L * L / (8.0 * (TC.SPHERE_R - L))
    dist = np.abs(np.linalg.norm(V.astype(np.float64) - TC.SPHERE_C, axis=1) - TC.SPHERE_R)
    print(f"sphere: {len(V)} vertices, {len(F)} faces, max distance {dist.max():.4f}, bound {bound:.4f}")
    assert dist.max() <= bound + 1e-5
    assert np.abs(C - V / np.float32(20.0) * [1, 1, 0.5] - [0, 0, 0.25]).max() < 1e-5      # the colour field is linear: interpolation keeps it


def test_torus_mesh_is_a_closed_torus():
    V, _, F = TC.field_mesh("torus")
    assert TR.is_closed(F) and TR.euler(len(V), F) == 0 and TR.all_referenced(len(V), F)


def test_plane_mesh_ends_where_the_weight_does():
    V, _, F = TC.field_mesh("plane")
    assert len(F) > 0 and V[:, 0].max() <= TC.PLANE_X_MAX
    de = TR.directed_edges(F)
    assert all(n == 1 for n in de.values())                       # oriented: no directed edge twice
    rim = TR.open_edges(F)
    assert rim and TR.euler(len(V), F) == 1                       # a disc
    top = np.array([TC.PLANE_X_MAX, TC.FIELD_DIMS[1] - 1, TC.FIELD_DIMS[2] - 1], dtype=np.float32)
    for a, b in rim:                                              # open edges only on the rim: both ends in one bounding plane
        on = ((V[a] == 0) & (V[b] == 0)) | ((V[a] == top) & (V[b] == top))
        assert on.any(), (V[a], V[b])
    n = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]).astype(np.float64)
    assert ((n @ TC.PLANE_N) > 0).all()                           # from inside (f < 0) to outside


def test_exact_zeros_leave_the_sphere_closed():
    """What catches a winding decided from computed positions: samples that are exactly 0 give triangles of zero area."""
    vol = TC.field("sphere_zeroed")
    assert (vol.tsdf == 0).sum() > 50
    V, _, F = TC.field_mesh("sphere_zeroed")
    assert TR.is_closed(F) and TR.euler(len(V), F) == 2 and TR.all_referenced(len(V), F)
    tri = V[F].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (area == 0).any()


def test_thin_and_empty_fields():
    V, _, F = TC.field_mesh("thin")
    assert len(F) > 0 and TR.all_referenced(len(V), F) and all(n == 1 for n in TR.directed_edges(F).values())
    V, C, F = TC.field_mesh("empty")
    assert V.shape == (0, 3) and C.shape == (0, 3) and F.shape == (0, 3)


def test_wide_field_needs_more_than_one_round_of_the_block_sum_scan():
    V, _, F = TC.field_mesh("wide")
    assert 7 * int(np.prod(TC.WIDE_DIMS)) > 256 * 2048
    assert TR.is_closed(F) and TR.euler(len(V), F) == 2 and TR.all_referenced(len(V), F)


def test_end_to_end_reference_mesh_is_closed():
    _, (V, _, F) = TC.e2e_reference()
    assert TR.is_closed(F) and TR.euler(len(V), F) == 2
    r = np.linalg.norm(V.astype(np.float64) - TC.E2E_SPHERE_C, axis=1)
    assert np.abs(r - TC.E2E_SPHERE_R).max() < TC.E2E_S           # on the sphere to within a voxel


# ---- pinhole_of ------------------------------------------------------------------------------------------------------------------
def _proj64(cam):
    """The rasterizer's projection matrix (cameras.projection_matrix) in float64, row-vector convention."""
    tx, ty = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    n, f = cam.znear, cam.zfar
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[3, 2] = 1.0 / tx, 1.0 / ty, 1.0
    P[2, 2], P[2, 3] = f / (f - n), -(f * n) / (f - n)
    return P.T


@pytest.mark.parametrize("pose", sorted(posed_cases.POSES))
def test_pinhole_of_agrees_with_the_rasterizers_projection(pose):
    from luciddreamer_amd import tsdf
    W, H = 131, 77
    cam = posed_cases.camera(pose, W, H)
    K, R, T = tsdf.pinhole_of(cam)
    assert K.dtype == R.dtype == T.dtype == np.float64 and K.shape == (3, 3) and R.shape == (3, 3) and T.shape == (3,)
    rng = np.random.default_rng(5)
    view = cam.world_view_transform.double().numpy()
    cam_pts = np.stack([rng.uniform(-2, 2, 200), rng.uniform(-1.5, 1.5, 200), rng.uniform(0.5, 6.0, 200)], axis=1)
    X = (cam_pts - view[3, :3]) @ np.linalg.inv(view[:3, :3])        # world points in front of the camera
    p = X @ R.T + T
    q = p @ K.T
    uv = q[:, :2] / q[:, 2:3]
    for full, tol in ((view @ _proj64(cam), 1e-9), (cam.full_proj_transform.double().numpy(), 2e-3)):     # float64; as stored
        h = np.concatenate([X, np.ones((len(X), 1))], axis=1) @ full
        ndc = h[:, :2] / h[:, 3:4]
        pix = ((ndc + 1.0) * [W, H] - 1.0) / 2.0
        print(f"{pose}: max pixel difference {np.abs(pix - uv).max():.3e} (bound {tol})")
        assert np.abs(pix - uv).max() <= tol
    assert np.allclose(p, cam_pts, atol=1e-12)


# ---- the C ABI on a machine without a device -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


SYMBOLS = ("lr_tsdf_workspace_bytes", "lr_tsdf_integrate", "lr_tsdf_extract_count", "lr_tsdf_extract_emit")


def test_symbols_are_exported(L):
    from luciddreamer_amd import _lib, build
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert build.SOURCES["tsdf.hip"] == ["-ffp-contract=off"]


@pytest.mark.parametrize("struct, cname", [("TsdfIntegrateArgs", "lr_tsdf_integrate_args"), ("TsdfExtractArgs", "lr_tsdf_extract_args"),
                                           ("TsdfVolumeDesc", "lr_tsdf_volume")])
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
                           for n, _, _ in members) +
                   "    return 0;\n}\n")
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


_BUF = (ctypes.c_double * 72)()
PTR = (ctypes.addressof(_BUF) + 15) & ~15               # non-NULL, 16-byte aligned, never dereferenced by the checks
_EYE = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
_ZERO = (ctypes.c_double * 3)(0, 0, 0)
_COUNTS = (ctypes.c_longlong * 2)()
NAN, INF = float("nan"), float("inf")


def _mat(values):
    return (ctypes.c_double * len(values))(*values)


def _vol(**fields):
    from luciddreamer_amd import _lib
    v = dict(origin=(ctypes.c_float * 3)(0, 0, 0), voxel_size=0.1, nx=20, ny=18, nz=16, trunc=0.3, tsdf=PTR, weight=PTR, color=PTR)
    v.update(fields)
    return _lib.TsdfVolumeDesc(**v)


def _split(fields):
    vol = {k[4:]: v for k, v in fields.items() if k.startswith("vol_")}
    rest = {k: v for k, v in fields.items() if not k.startswith("vol_")}
    return vol, rest


def _integrate_args(**fields):
    from luciddreamer_amd import _lib
    vol, rest = _split(fields)
    a = dict(vol=_vol(**vol), n_frames=1, height=24, width=32, depth=PTR, color=PTR, pixel_weight=PTR, K=_EYE, R=_EYE, T=_ZERO,
             depth_max=INF, max_weight=INF)
    a.update(rest)
    keep = [v for v in a.values() if isinstance(v, ctypes.Array)]
    a = {k: (ctypes.addressof(v) if isinstance(v, ctypes.Array) else v) for k, v in a.items()}
    s = _lib.TsdfIntegrateArgs(**a)
    s._keep = keep
    return s


def _extract_args(**fields):
    from luciddreamer_amd import _lib
    vol, rest = _split(fields)
    a = dict(vol=_vol(**vol), min_weight=1.0, workspace=PTR, workspace_bytes=1 << 40, out_n_vertices=ctypes.addressof(_COUNTS),
             out_n_faces=ctypes.addressof(_COUNTS) + 8, n_vertices=10, n_faces=10, out_vertices=PTR, out_colors=PTR, out_faces=PTR)
    a.update(rest)
    return _lib.TsdfExtractArgs(**a)


_ORIGIN_NAN = (ctypes.c_float * 3)(0, NAN, 0)
VOLUME_REJECTED = {
    "nx_1": (dict(vol_nx=1), b"nx, ny, nz"),
    "ny_0": (dict(vol_ny=0), b"nx, ny, nz"),
    "nz_negative": (dict(vol_nz=-4), b"nx, ny, nz"),
    "edges_beyond_int": (dict(vol_nx=1024, vol_ny=1024, vol_nz=293), b"2^31"),
    "dims_overflow_int": (dict(vol_nx=65536, vol_ny=65536, vol_nz=65536), b"2^31"),
    "zero_voxel": (dict(vol_voxel_size=0.0), b"voxel_size and trunc"),
    "nan_voxel": (dict(vol_voxel_size=NAN), b"voxel_size and trunc"),
    "inf_voxel": (dict(vol_voxel_size=INF), b"voxel_size and trunc"),
    "negative_trunc": (dict(vol_trunc=-0.3), b"voxel_size and trunc"),
    "nan_trunc": (dict(vol_trunc=NAN), b"voxel_size and trunc"),
    "inf_trunc": (dict(vol_trunc=INF), b"voxel_size and trunc"),
    "nan_origin": (dict(vol_origin=_ORIGIN_NAN), b"origin"),
    "no_tsdf": (dict(vol_tsdf=None), b"tsdf, weight and color are required"),
    "no_weight": (dict(vol_weight=None), b"tsdf, weight and color are required"),
    "no_color_volume": (dict(vol_color=None), b"tsdf, weight and color are required"),
    "misaligned_tsdf": (dict(vol_tsdf=PTR + 4), b"16-byte aligned"),
    "misaligned_weight": (dict(vol_weight=PTR + 8), b"16-byte aligned"),
    "misaligned_color_volume": (dict(vol_color=PTR + 12), b"16-byte aligned"),
}
INTEGRATE_REJECTED = dict(VOLUME_REJECTED, **{
    "no_frames": (dict(n_frames=0), b"n_frames"),
    "too_many_frames": (dict(n_frames=65536), b"n_frames"),
    "height_1": (dict(height=1), b"height and width"),
    "pixels_beyond_int": (dict(height=65536, width=65536), b"H*W"),
    "no_K": (dict(K=None), b"K, R and T are required"),
    "no_R": (dict(R=None), b"K, R and T are required"),
    "no_T": (dict(T=None), b"K, R and T are required"),
    "nan_K": (dict(K=_mat([1, 0, 0, 0, NAN, 0, 0, 0, 1])), b"finite"),
    "inf_R_second_frame": (dict(n_frames=2, R=_mat([1, 0, 0, 0, 1, 0, 0, 0, 1] + [1, 0, 0, 0, 1, 0, 0, INF, 1]), T=_mat([0] * 6)), b"finite"),
    "nan_T_second_frame": (dict(n_frames=2, R=_mat([1, 0, 0, 0, 1, 0, 0, 0, 1] * 2), T=_mat([0, 0, 0, 0, NAN, 0])), b"finite"),
    "nan_depth_max": (dict(depth_max=NAN), b"depth_max and max_weight"),
    "zero_depth_max": (dict(depth_max=0.0), b"depth_max and max_weight"),
    "nan_max_weight": (dict(max_weight=NAN), b"depth_max and max_weight"),
    "negative_max_weight": (dict(max_weight=-1.0), b"depth_max and max_weight"),
    "no_depth": (dict(depth=None), b"depth is required"),
    "misaligned_depth": (dict(depth=PTR + 4), b"16-byte aligned"),
    "misaligned_color": (dict(color=PTR + 8), b"16-byte aligned"),
    "misaligned_pixel_weight": (dict(pixel_weight=PTR + 4), b"16-byte aligned"),
})
EXTRACT_REJECTED = dict(VOLUME_REJECTED, **{
    "no_workspace": (dict(workspace=None), b"workspace"),
    "misaligned_workspace": (dict(workspace=PTR + 8), b"workspace"),
    "small_workspace": (dict(workspace_bytes=20 * 18 * 16 * 40 - 1), b"workspace"),
})
COUNT_REJECTED = dict(EXTRACT_REJECTED, **{
    "nan_min_weight": (dict(min_weight=NAN), b"min_weight"),
    "no_vertex_count": (dict(out_n_vertices=None), b"out_n_vertices and out_n_faces"),
    "no_face_count": (dict(out_n_faces=None), b"out_n_vertices and out_n_faces"),
})
EMIT_REJECTED = dict(EXTRACT_REJECTED, **{
    "negative_vertices": (dict(n_vertices=-1), b"n_vertices and n_faces"),
    "negative_faces": (dict(n_faces=-1), b"n_vertices and n_faces"),
    "faces_beyond_int": (dict(n_faces=(1 << 31) // 3 + 1), b"n_vertices and n_faces"),
    "no_vertices": (dict(out_vertices=None), b"are required"),
    "no_colors": (dict(out_colors=None), b"are required"),
    "no_faces": (dict(out_faces=None), b"are required"),
    "misaligned_vertices": (dict(out_vertices=PTR + 4), b"16-byte aligned"),
    "misaligned_colors": (dict(out_colors=PTR + 4), b"16-byte aligned"),
    "misaligned_faces": (dict(out_faces=PTR + 4), b"16-byte aligned"),
})


def _refused(L, fn, args, message):
    from luciddreamer_amd import _lib
    assert fn(args) == _lib.LR_ERR_INVALID_ARG
    assert message in L.lr_last_error(), L.lr_last_error()


@pytest.mark.parametrize("case", sorted(INTEGRATE_REJECTED))
def test_integrate_rejects_without_a_device(L, case):
    fields, message = INTEGRATE_REJECTED[case]
    _refused(L, L.lr_tsdf_integrate, _integrate_args(**fields), message)


@pytest.mark.parametrize("case", sorted(COUNT_REJECTED))
def test_extract_count_rejects_without_a_device(L, case):
    fields, message = COUNT_REJECTED[case]
    _refused(L, L.lr_tsdf_extract_count, _extract_args(**fields), message)


@pytest.mark.parametrize("case", sorted(EMIT_REJECTED))
def test_extract_emit_rejects_without_a_device(L, case):
    fields, message = EMIT_REJECTED[case]
    _refused(L, L.lr_tsdf_extract_emit, _extract_args(**fields), message)


@pytest.mark.parametrize("delta", [-1, 1, -8, 8])
def test_struct_bytes_is_checked_first(L, delta):
    from luciddreamer_amd import _lib
    for fn, make in ((L.lr_tsdf_integrate, _integrate_args), (L.lr_tsdf_extract_count, _extract_args),
                     (L.lr_tsdf_extract_emit, _extract_args)):
        assert fn(None) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
        a = make(vol_nx=0, vol_tsdf=None)                            # everything else is wrong as well
        a.struct_bytes += delta
        assert fn(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    a = _extract_args()
    a.struct_bytes += delta
    assert L.lr_tsdf_workspace_bytes(a) == 0 and L.lr_tsdf_workspace_bytes(None) == 0


def test_workspace_size_is_a_pure_host_function(L):
    w = lambda nx, ny, nz: L.lr_tsdf_workspace_bytes(_extract_args(vol_nx=nx, vol_ny=ny, vol_nz=nz))
    assert w(20, 18, 16) >= 20 * 18 * 16 * 40 and w(20, 18, 16) % 256 == 0
    assert w(20, 18, 16) < w(21, 18, 16) < w(21, 19, 16) < w(21, 19, 17)
    assert w(1, 18, 16) == 0 and w(1024, 1024, 293) == 0 and w(65536, 65536, 65536) == 0
    assert w(1024, 1024, 292) > 0


# ---- the public interface ----------------------------------------------------------------------------------------------------
def test_package_exports_the_module():
    import luciddreamer_amd
    t = luciddreamer_amd.tsdf
    for name in ("TSDFVolume", "pinhole_of", "fuse_views", "save_mesh_ply"):
        assert hasattr(t, name), name
    for name in ("integrate", "integrate_batch", "extract_mesh", "reset"):
        assert hasattr(t.TSDFVolume, name), name


def test_frames_per_group_is_the_kernels_frames_per_launch():
    import re
    from luciddreamer_amd import tsdf
    text = open(os.path.join(ROOT, "luciddreamer_amd", "csrc", "common.h")).read()
    assert int(re.search(r"REPROJECT_FRAMES_PER_LAUNCH = (\d+);", text).group(1)) == tsdf.FRAMES_PER_GROUP


def test_wrong_sized_poses_name_this_module():
    from luciddreamer_amd import tsdf
    with pytest.raises(ValueError, match="^tsdf: K must hold"):
        tsdf._host64(np.eye(4), (3, 3), "K")


def test_host_volume_raises():
    from luciddreamer_amd import tsdf
    with pytest.raises(RuntimeError, match="HIP device"):
        tsdf.TSDFVolume((0, 0, 0), 0.1, (8, 8, 8), 0.3, "cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        tsdf._dense(torch.zeros(2, 4, 4), (2, 4, 4), torch.device("cuda", 0), "depth")


def test_save_mesh_ply_layout(tmp_path):
    from luciddreamer_amd import tsdf
    V, C, F = TC.field_mesh("thin")
    path = tmp_path / "m.ply"
    tsdf.save_mesh_ply(str(path), torch.from_numpy(V), torch.from_numpy(C), torch.from_numpy(F))
    raw = path.read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n")
    assert f"element vertex {len(V)}".encode() in head and f"element face {len(F)}".encode() in head
    assert len(body) == len(V) * 15 + len(F) * 13
