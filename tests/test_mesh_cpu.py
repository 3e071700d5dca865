"""Mesh clean-up without a device: the numpy restatement (tests/mesh_ref.py) is sound -- its labels are SciPy's components, the
seeded cases are what their comments say, the filter's rules hold on them --, the ctypes mirrors match the header, and the C ABI
refuses every bad argument in front of its first HIP call."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import mesh_cases as MC
from tests import mesh_ref as MR
from tests import tsdf_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement: components ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.ALL_NAMES)
def test_labels_are_scipys_components(name):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    v, _, f = MC.mesh(name)
    V = len(v)
    face_labels, vertex_labels, labels, counts = MC.components_reference(name)
    g = f[MR.in_range(f, V)].astype(np.int64)
    rows, cols = np.concatenate([g[:, 0], g[:, 0]]), np.concatenate([g[:, 1], g[:, 2]])
    _, comp = connected_components(sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V)), directed=False)
    # the smallest vertex index of each of SciPy's components
    smallest = np.full(comp.max() + 1 if V else 0, V, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(V))
    assert np.array_equal(vertex_labels, smallest[comp].astype(np.int32))
    assert np.array_equal(face_labels[face_labels >= 0], vertex_labels[g[:, 0]])
    assert (face_labels >= 0).sum() == len(g) == counts.sum()


@pytest.mark.parametrize("name", MC.ALL_NAMES)
def test_labels_are_canonical(name):
    v, _, f = MC.mesh(name)
    face_labels, vertex_labels, labels, counts = MC.components_reference(name)
    assert (vertex_labels <= np.arange(len(v))).all() and np.array_equal(vertex_labels[vertex_labels], vertex_labels)
    assert np.array_equal(labels, np.unique(face_labels[face_labels >= 0])) and (counts > 0).all()
    referenced = np.zeros(len(v), dtype=bool)
    referenced[f[face_labels >= 0].reshape(-1)] = True
    assert np.array_equal(vertex_labels[~referenced], np.arange(len(v))[~referenced])     # unreferenced: its own label


def _by_size(labels, counts):
    order = np.argsort(-counts.astype(np.int64), kind="stable")
    return counts[order], labels[order]


def test_blobs_is_the_pinned_case():
    v, c, f = MC.field_mesh("blobs")
    assert (len(v), len(f)) == (MC.BLOBS_V, MC.BLOBS_T)
    face_labels, vertex_labels, labels, counts = MC.components_reference("blobs")
    counts, labels = _by_size(labels, counts)
    assert tuple(counts) == MC.BLOBS_COUNTS and tuple(labels) == MC.BLOBS_LABELS
    for label in MC.BLOBS_LABELS:                                     # every blob is a closed sphere of its own
        assert MR.component_euler(len(v), f, face_labels, label) == 2
    assert TR.is_closed(f)


@pytest.mark.parametrize("name", MC.FIELD_NAMES)
def test_field_meshes_are_what_the_cases_say(name):
    v, c, f = MC.field_mesh(name)
    zero_area, n_components = MC.FIELD_FACTS[name]
    face_labels, _, labels, counts = MC.components_reference(name)
    assert len(labels) == n_components
    if name == "empty":
        assert len(v) == 0 and len(f) == 0
        return
    _, L = MR.face_cross(v, f)
    assert int((~(np.isfinite(L) & (L > 0))).sum()) == zero_area
    if name == "thin":
        assert tuple(_by_size(labels, counts)[0][:5]) == MC.THIN_LARGEST
    if name == "sphere":                                             # outward winding on every face
        tri = v[f].astype(np.float64)
        n, _ = MR.face_cross(v, f)
        assert ((n * (tri.mean(axis=1) - MC.tsdf_cases.SPHERE_C)).sum(axis=1) > 0).all()


def test_synthetic_meshes_are_what_the_cases_say():
    for name, T in (("strip", 5000), ("long_strip", 530000), ("ordered_strip", 200000)):
        v, f = MC.synthetic(name)
        assert len(f) == T and len(MC.components_reference(name)[2]) == 1
    assert -(-530000 // 2048) > 256                                  # a second round of the block-sum scan
    v, f = MC.synthetic("forest")
    assert len(f) == 3001 and len(MC.components_reference("forest")[2]) == 3001
    assert all(3001 % m for m in (64, 256, 2048))
    v, f = MC.synthetic("fan")
    assert (f == 7).any(axis=1).all() and len(f) == 3000 > 2048
    v, f = MC.synthetic("mixed")
    V = len(v)
    assert (f == -1).any() and (f == V).any() and (f == 2 ** 31 - 1).any()
    assert np.isnan(v).any() and np.isinf(v).any()
    ok = MR.in_range(f, V)
    g = f[ok]
    assert ((g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2])).any()
    assert len(np.unique(g, axis=0)) < len(g)                        # duplicate faces
    assert len(np.unique(g)) < V                                     # unreferenced vertices


# ---- the restatement: filter ----------------------------------------------------------------------------------------------------
def test_filter_rules_on_blobs():
    v, c, f = MC.field_mesh("blobs")
    kept = {s: len(MC.filter_reference("blobs", s)["faces"]) for s in MC.FILTER_SETTINGS}
    assert kept[(0, 1, False)] == MC.BLOBS_T and kept[(1, 1, False)] == 5772
    assert kept[(2, 1, False)] == 7916 == kept[(3, 1, False)]        # the tie: three components
    assert kept[(100, 1, False)] == MC.BLOBS_T                       # K > C
    assert kept[(0, 100, False)] == 5772 + 1072 + 1072 + 408 + 144
    assert kept[(2, 2000, False)] == 5772                            # M above kth
    assert kept[(0, 10 ** 9, False)] == 0 and len(MC.filter_reference("blobs", (0, 10 ** 9, False))["vertices"]) == 0
    r = MC.filter_reference("blobs", (0, 1, False))
    assert np.array_equal(r["vertices"], v) and np.array_equal(r["faces"], f)        # the identity


@pytest.mark.parametrize("name", MC.FILTER_MESHES)
@pytest.mark.parametrize("setting", MC.FILTER_SETTINGS)
def test_filter_restatement_properties(name, setting):
    v, c, f = MC.mesh(name)
    r = MC.filter_reference(name, setting)
    assert np.array_equal(r["vertices"].view(np.uint32), v[r["vertex_index"]].view(np.uint32))
    assert (np.diff(r["vertex_index"]) > 0).all() and (np.diff(r["face_index"]) > 0).all()        # input order
    assert np.array_equal(r["vertex_index"][r["faces"]], f[r["face_index"]])
    assert TR.all_referenced(len(r["vertices"]), r["faces"]) or len(r["vertices"]) == 0
    K, M, dd = setting
    again = MR.filter_clusters(r["vertices"], r["faces"], keep_largest=K, min_faces=M, drop_degenerate=dd)
    assert np.array_equal(again["faces"], r["faces"]) and len(again["vertices"]) == len(r["vertices"])
    if dd and name in ("thin", "sphere_zeroed"):
        assert len(r["vertices"]) < len(v) and len(r["faces"]) == len(f) - MC.FIELD_FACTS[name][0]


# ---- the restatement: normals ---------------------------------------------------------------------------------------------------
def test_normals_restatement():
    v, c, f = MC.field_mesh("sphere")
    n = MC.normals_reference("sphere")
    assert ((n.astype(np.float64) * (v - MC.tsdf_cases.SPHERE_C)).sum(axis=1) > 0).all()
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    v, f = MC.synthetic("mixed")
    n = MC.normals_reference("mixed")
    referenced = np.zeros(len(v), dtype=bool)
    referenced[f[MR.in_range(f, len(v))].reshape(-1)] = True
    assert (~referenced).any() and (n[~referenced] == 0).all() and np.isfinite(n).all()
    v, f = MC.synthetic("fan")
    perm = np.random.default_rng(1).permutation(len(f))
    assert np.array_equal(MR.vertex_normals(v, f[perm]).view(np.uint32), MC.normals_reference("fan").view(np.uint32))


# ---- the C ABI on a machine without a device ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


SYMBOLS = ("lr_mesh_workspace_bytes", "lr_mesh_components", "lr_mesh_filter_count", "lr_mesh_filter_emit",
           "lr_mesh_vertex_normals")


def test_symbols_are_exported(L):
    from luciddreamer_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "lucid_raster.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS and name + "(" in header, name
    assert build.SOURCES["mesh.hip"] == ["-ffp-contract=off"]


@pytest.mark.parametrize("struct, cname", [("MeshComponentsArgs", "lr_mesh_components_args"),
                                           ("MeshFilterArgs", "lr_mesh_filter_args"), ("MeshNormalsArgs", "lr_mesh_normals_args")])
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
_COUNTS = (ctypes.c_longlong * 2)()
LIMIT = 2 ** 31 - 2 ** 12


def _components_args(**fields):
    from luciddreamer_amd import _lib
    a = dict(n_vertices=100, n_faces=50, faces=PTR, vertex_labels=PTR, face_labels=PTR, component_faces=PTR, workspace=PTR,
             workspace_bytes=1 << 40)
    a.update(fields)
    return _lib.MeshComponentsArgs(**a)


def _filter_args(**fields):
    from luciddreamer_amd import _lib
    a = dict(n_vertices=100, n_faces=50, vertices=PTR, faces=PTR, colors=PTR, normals=PTR, keep_largest=2, min_faces=1,
             drop_degenerate=1, workspace=PTR, workspace_bytes=1 << 40, out_n_vertices=ctypes.addressof(_COUNTS),
             out_n_faces=ctypes.addressof(_COUNTS) + 8, n_out_vertices=10, n_out_faces=10, out_vertices=PTR, out_colors=PTR,
             out_normals=PTR, out_faces=PTR, out_vertex_index=PTR, out_face_index=PTR)
    a.update(fields)
    return _lib.MeshFilterArgs(**a)


def _normals_args(**fields):
    from luciddreamer_amd import _lib
    a = dict(n_vertices=100, n_faces=50, vertices=PTR, faces=PTR, out_normals=PTR, workspace=PTR, workspace_bytes=1 << 40)
    a.update(fields)
    return _lib.MeshNormalsArgs(**a)


COMMON_REJECTED = {
    "negative_vertices": (dict(n_vertices=-1), b"n_vertices and n_faces"),
    "negative_faces": (dict(n_faces=-1), b"n_vertices and n_faces"),
    "too_many_vertices": (dict(n_vertices=LIMIT + 1), b"2^31"),
    "too_many_faces": (dict(n_faces=LIMIT + 1), b"2^31"),
    "no_faces": (dict(faces=None), b"faces is required"),
    "misaligned_faces": (dict(faces=PTR + 4), b"16-byte aligned"),
    "no_workspace": (dict(workspace=None), b"workspace"),
    "misaligned_workspace": (dict(workspace=PTR + 8), b"workspace"),
    "small_workspace": (dict(workspace_bytes=100 * 24 + 50 * 9 - 1), b"workspace"),
}
COMPONENTS_REJECTED = dict(COMMON_REJECTED, **{
    "no_vertex_labels": (dict(vertex_labels=None), b"are required"),
    "no_face_labels": (dict(face_labels=None), b"are required"),
    "no_component_faces": (dict(component_faces=None), b"are required"),
    "misaligned_vertex_labels": (dict(vertex_labels=PTR + 4), b"16-byte aligned"),
    "misaligned_face_labels": (dict(face_labels=PTR + 8), b"16-byte aligned"),
})
FILTER_REJECTED = dict(COMMON_REJECTED, **{
    "negative_keep_largest": (dict(keep_largest=-1), b"keep_largest must be >= 0"),
    "zero_min_faces": (dict(min_faces=0), b"min_faces must be >= 1"),
    "negative_min_faces": (dict(min_faces=-5), b"min_faces must be >= 1"),
    "no_vertices": (dict(vertices=None), b"vertices is required"),
    "misaligned_vertices": (dict(vertices=PTR + 4), b"16-byte aligned"),
    "misaligned_colors": (dict(colors=PTR + 8), b"16-byte aligned"),
    "misaligned_normals": (dict(normals=PTR + 12), b"16-byte aligned"),
})
COUNT_REJECTED = dict(FILTER_REJECTED, **{
    "no_vertex_count": (dict(out_n_vertices=None), b"out_n_vertices and out_n_faces"),
    "no_face_count": (dict(out_n_faces=None), b"out_n_vertices and out_n_faces"),
})
EMIT_REJECTED = dict(FILTER_REJECTED, **{
    "negative_out_vertices": (dict(n_out_vertices=-1), b"n_out_vertices and n_out_faces"),
    "negative_out_faces": (dict(n_out_faces=-1), b"n_out_vertices and n_out_faces"),
    "more_out_vertices_than_vertices": (dict(n_out_vertices=101), b"n_out_vertices and n_out_faces"),
    "more_out_faces_than_faces": (dict(n_out_faces=51), b"n_out_vertices and n_out_faces"),
    "no_out_vertices": (dict(out_vertices=None), b"are required"),
    "no_out_faces": (dict(out_faces=None), b"are required"),
    "no_out_colors": (dict(out_colors=None), b"are required"),
    "no_out_normals": (dict(out_normals=None), b"are required"),
    "misaligned_out_vertices": (dict(out_vertices=PTR + 4), b"16-byte aligned"),
    "misaligned_out_faces": (dict(out_faces=PTR + 4), b"16-byte aligned"),
    "misaligned_out_vertex_index": (dict(out_vertex_index=PTR + 4), b"16-byte aligned"),
    "misaligned_out_face_index": (dict(out_face_index=PTR + 8), b"16-byte aligned"),
})
NORMALS_REJECTED = dict(COMMON_REJECTED, **{
    "no_vertices": (dict(vertices=None), b"are required"),
    "no_out_normals": (dict(out_normals=None), b"are required"),
    "misaligned_vertices": (dict(vertices=PTR + 4), b"16-byte aligned"),
    "misaligned_out_normals": (dict(out_normals=PTR + 8), b"16-byte aligned"),
})


def _refused(L, fn, args, message):
    from luciddreamer_amd import _lib
    assert fn(args) == _lib.LR_ERR_INVALID_ARG
    assert message in L.lr_last_error(), L.lr_last_error()


@pytest.mark.parametrize("case", sorted(COMPONENTS_REJECTED))
def test_components_rejects_without_a_device(L, case):
    fields, message = COMPONENTS_REJECTED[case]
    _refused(L, L.lr_mesh_components, _components_args(**fields), message)


@pytest.mark.parametrize("case", sorted(COUNT_REJECTED))
def test_filter_count_rejects_without_a_device(L, case):
    fields, message = COUNT_REJECTED[case]
    _refused(L, L.lr_mesh_filter_count, _filter_args(**fields), message)


@pytest.mark.parametrize("case", sorted(EMIT_REJECTED))
def test_filter_emit_rejects_without_a_device(L, case):
    fields, message = EMIT_REJECTED[case]
    _refused(L, L.lr_mesh_filter_emit, _filter_args(**fields), message)


@pytest.mark.parametrize("case", sorted(NORMALS_REJECTED))
def test_vertex_normals_rejects_without_a_device(L, case):
    fields, message = NORMALS_REJECTED[case]
    _refused(L, L.lr_mesh_vertex_normals, _normals_args(**fields), message)


@pytest.mark.parametrize("delta", [-1, 1, -8, 8])
def test_struct_bytes_is_checked_first(L, delta):
    from luciddreamer_amd import _lib
    for fn, make in ((L.lr_mesh_components, _components_args), (L.lr_mesh_filter_count, _filter_args),
                     (L.lr_mesh_filter_emit, _filter_args), (L.lr_mesh_vertex_normals, _normals_args)):
        assert fn(None) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
        a = make(n_vertices=-1, faces=None)                          # everything else is wrong as well
        a.struct_bytes += delta
        assert fn(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()


def test_empty_meshes_return_without_a_device(L):
    """V = 0 and T = 0 need no pointer and no launch: the calls return 0 on a machine without a device."""
    none = dict(n_vertices=0, n_faces=0, faces=None, workspace=None, workspace_bytes=0)
    assert L.lr_mesh_components(_components_args(vertex_labels=None, face_labels=None, component_faces=None, **none)) == 0
    assert L.lr_mesh_vertex_normals(_normals_args(vertices=None, out_normals=None, **none)) == 0
    _COUNTS[0], _COUNTS[1] = 7, 7
    a = _filter_args(vertices=None, colors=None, normals=None, n_out_vertices=0, n_out_faces=0, out_vertices=None,
                     out_colors=None, out_normals=None, out_faces=None, out_vertex_index=None, out_face_index=None, **none)
    assert L.lr_mesh_filter_count(a) == 0 and (_COUNTS[0], _COUNTS[1]) == (0, 0)
    assert L.lr_mesh_filter_emit(a) == 0
    # vertices without faces: nothing is kept, nothing is launched
    _COUNTS[0], _COUNTS[1] = 7, 7
    assert L.lr_mesh_filter_count(_filter_args(n_faces=0, faces=None)) == 0 and (_COUNTS[0], _COUNTS[1]) == (0, 0)


def test_workspace_size_is_a_pure_host_function(L):
    w = L.lr_mesh_workspace_bytes
    assert w(100, 50) >= 100 * 24 + 50 * 9 and w(100, 50) % 256 == 0
    assert w(1000, 50) < w(2000, 50) < w(2000, 5000) and w(0, 0) > 0
    assert w(-1, 5) == 0 and w(5, -1) == 0 and w(LIMIT + 1, 5) == 0 and w(5, LIMIT + 1) == 0
    assert w(LIMIT, LIMIT) >= LIMIT * 33


# ---- the public interface -------------------------------------------------------------------------------------------------------
def test_package_exports_the_module():
    import luciddreamer_amd
    m = luciddreamer_amd.mesh
    for name in ("connected_components", "filter_clusters", "vertex_normals", "post_process"):
        assert callable(getattr(m, name)), name


def test_host_tensors_raise():
    from luciddreamer_amd import mesh
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh.connected_components(f, 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh.filter_clusters(v, f)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh.vertex_normals(v, f)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh.post_process(v, v, f)
    with pytest.raises(TypeError, match="torch.Tensor"):
        mesh.vertex_normals(v.numpy(), f)


# ---- the file -------------------------------------------------------------------------------------------------------------------
def _earlier_writer(path, vertices, colors, faces):
    """save_mesh_ply as it was before it took normals."""
    v, c, f = vertices.astype(np.float32), colors.astype(np.float32), faces.astype(np.int32)
    c8 = np.rint(np.clip(np.nan_to_num(c, nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
    vrec = np.empty(v.shape[0], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    vrec["xyz"], vrec["rgb"] = v, c8
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", 3)])
    frec["n"], frec["idx"] = 3, f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii") + vrec.tobytes() + frec.tobytes())


def read_ply(path):
    """(xyz, normals or None, rgb, faces) of a file save_mesh_ply wrote: a minimal reader."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
    xyz = [["float", "x"], ["float", "y"], ["float", "z"]]
    nrm = [["float", "nx"], ["float", "ny"], ["float", "nz"]]
    tail = [["uchar", "red"], ["uchar", "green"], ["uchar", "blue"], ["list", "uchar", "int", "vertex_indices"]]
    with_normals = props == xyz + nrm + tail
    assert with_normals or props == xyz + tail
    fields = [("xyz", "<f4", 3)] + ([("nxyz", "<f4", 3)] if with_normals else []) + [("rgb", "u1", 3)]
    vdt = np.dtype(fields)
    v = np.frombuffer(body, dtype=vdt, count=nv)
    f = np.frombuffer(body, dtype=np.dtype([("n", "u1"), ("idx", "<i4", 3)]), count=nf, offset=nv * vdt.itemsize)
    assert len(body) == nv * vdt.itemsize + nf * 13 and (f["n"] == 3).all()
    return v["xyz"], v["nxyz"] if with_normals else None, v["rgb"], f["idx"]


def test_save_mesh_ply_with_and_without_normals(tmp_path):
    from luciddreamer_amd import tsdf
    V, C, F = MC.field_mesh("blobs")
    N = MC.normals_reference("blobs")
    t = lambda a: torch.from_numpy(np.array(a))
    plain, earlier, with_normals = (str(tmp_path / n) for n in ("plain.ply", "earlier.ply", "normals.ply"))
    tsdf.save_mesh_ply(plain, t(V), t(C), t(F))
    _earlier_writer(earlier, V, C, F)
    assert open(plain, "rb").read() == open(earlier, "rb").read()     # without normals: the same bytes as before
    tsdf.save_mesh_ply(with_normals, t(V), t(C), t(F), normals=t(N))
    xyz, nrm, rgb, idx = read_ply(with_normals)
    assert np.array_equal(xyz.view(np.uint32), V.view(np.uint32)) and np.array_equal(nrm.view(np.uint32), N.view(np.uint32))
    assert np.array_equal(idx, F) and np.array_equal(rgb, read_ply(plain)[2])
    with pytest.raises(ValueError, match="normals"):
        tsdf.save_mesh_ply(with_normals, t(V), t(C), t(F), normals=t(N[:-1]))
