"""Mesh clean-up on the device against the numpy restatement (tests/mesh_ref.py), bit for bit: labels and counts, the filtered
rows with their attributes and index maps, vertex normals; repeatability and independence of the face order; TSDF volume to
cleaned mesh to PLY file end to end; the tensor hand-off."""
import numpy as np
import pytest
import torch

from tests import mesh_cases as MC
from tests import mesh_ref as MR
from tests import tsdf_ref as TR
from tests.test_mesh_cpu import read_ply

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(name, got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    differ = _bits(got) != _bits(want)
    if differ.any():
        with np.errstate(all="ignore"):
            print(f"{name}: {int(differ.sum())} of {differ.size} values differ, max |difference| "
                  f"{np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64))):.3e}")
    assert not differ.any(), name


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _permuted(faces, seed):
    return faces[np.random.default_rng(seed).permutation(len(faces))]


# ---- components -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.ALL_NAMES)
def test_components_equal_the_restatement(hip_device, name):
    from luciddreamer_amd import mesh
    v, _, f = MC.mesh(name)
    want = MC.components_reference(name)
    F = _dev(f, hip_device)
    got = mesh.connected_components(F, len(v))
    for t in got:
        assert t.device == F.device and t.dtype == torch.int32
    names = ("face_labels", "vertex_labels", "labels", "counts")
    for n, g, w in zip(names, got, want):
        _same_bits(n, g, w)
    again = mesh.connected_components(F, len(v))
    for n, g, w in zip(names, again, got):
        _same_bits(n + " (second run)", g, w.cpu().numpy())
    perm = mesh.connected_components(_dev(_permuted(f, 5), hip_device), len(v))
    _same_bits("vertex_labels (rows permuted)", perm[1], want[1])
    _same_bits("counts (rows permuted)", perm[3], want[3])


# ---- filter ---------------------------------------------------------------------------------------------------------------------
def _filter(mesh, v, c, n, f, setting, dev):
    K, M, dd = setting
    return mesh.filter_clusters(_dev(v, dev), _dev(f, dev), colors=_dev(c, dev), normals=_dev(n, dev), keep_largest=K,
                                min_faces=M, drop_degenerate=dd, return_index=True)


@pytest.mark.parametrize("name", MC.FILTER_MESHES)
@pytest.mark.parametrize("setting", MC.FILTER_SETTINGS)
def test_filter_equals_the_restatement(hip_device, name, setting):
    from luciddreamer_amd import mesh
    v, c, f = MC.mesh(name)
    n = MC.attribute_normals(name)
    want = MC.filter_reference(name, setting)
    out = _filter(mesh, v, c, n, f, setting, hip_device)
    if c is None:
        V2, F2, N2, vi, fi = out
        C2 = None
    else:
        V2, F2, C2, N2, vi, fi = out
        _same_bits("colors", C2, want["colors"])
    _same_bits("faces", F2, want["faces"])
    _same_bits("vertices", V2, want["vertices"])
    _same_bits("normals", N2, want["normals"])
    _same_bits("vertex_index", vi, want["vertex_index"])
    _same_bits("face_index", fi, want["face_index"])
    Vh, Fh, vih = V2.cpu().numpy(), F2.cpu().numpy(), vi.cpu().numpy()
    _same_bits("vertices against vertices[vertex_index]", Vh, v[vih])
    if setting == (0, 10 ** 9, False):
        assert Vh.shape == (0, 3) and Fh.shape == (0, 3)
    if len(Vh):
        assert TR.all_referenced(len(Vh), Fh)                                         # no kept vertex is unreferenced
    if setting == (2, 1, False) and name == "blobs":
        assert len(Fh) == 7916                                                        # the tie: three components kept
    if setting == (0, 1, True) and name in ("sphere_zeroed", "thin"):
        assert len(Vh) < len(v)                                                       # vertices drop out
    # filtering the result again with the same arguments changes nothing
    again = _filter(mesh, Vh, None if C2 is None else C2.cpu().numpy(), N2.cpu().numpy(), Fh, setting, hip_device)
    _same_bits("vertices (filtered again)", again[0], Vh)
    _same_bits("faces (filtered again)", again[1], Fh)
    _same_bits("vertex_index (filtered again)", again[-2], np.arange(len(Vh), dtype=np.int32))
    _same_bits("face_index (filtered again)", again[-1], np.arange(len(Fh), dtype=np.int32))


def test_filter_without_attributes_or_index(hip_device):
    from luciddreamer_amd import mesh
    v, c, f = MC.mesh("blobs")
    want = MC.filter_reference("blobs", (1, 1, False))
    out = mesh.filter_clusters(_dev(v, hip_device), _dev(f, hip_device), keep_largest=1)
    assert len(out) == 2
    _same_bits("vertices", out[0], want["vertices"])
    _same_bits("faces", out[1], want["faces"])
    V2, F2, C2 = mesh.filter_clusters(_dev(v, hip_device), _dev(f, hip_device), colors=_dev(c, hip_device), keep_largest=1)
    _same_bits("colors", C2, want["colors"])
    # beyond any int32 count: the same as no limit / as nothing kept
    big = mesh.filter_clusters(_dev(v, hip_device), _dev(f, hip_device), keep_largest=2 ** 40, min_faces=2 ** 40)
    assert big[0].shape == (0, 3) and big[1].shape == (0, 3)
    with pytest.raises(ValueError, match="keep_largest"):
        mesh.filter_clusters(_dev(v, hip_device), _dev(f, hip_device), keep_largest=-1)
    with pytest.raises(ValueError, match="min_faces"):
        mesh.filter_clusters(_dev(v, hip_device), _dev(f, hip_device), min_faces=0)


# ---- normals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.ALL_NAMES)
def test_normals_equal_the_restatement(hip_device, name):
    from luciddreamer_amd import mesh
    v, _, f = MC.mesh(name)
    want = MC.normals_reference(name)
    V = _dev(v, hip_device)
    got = mesh.vertex_normals(V, _dev(f, hip_device))
    assert got.device == V.device and got.dtype == torch.float32
    _same_bits("normals", got, want)
    _same_bits("normals (rows permuted)", mesh.vertex_normals(V, _dev(_permuted(f, 9), hip_device)), want)
    nh = got.cpu().numpy()
    referenced = np.zeros(len(v), dtype=bool)
    referenced[f[MR.in_range(f, len(v))].reshape(-1)] = True
    assert (nh[~referenced] == 0).all()                                               # zero for unreferenced vertices
    if name == "sphere":
        assert ((nh.astype(np.float64) * (v - MC.tsdf_cases.SPHERE_C)).sum(axis=1) > 0).all()
    if name == "mixed":
        assert (~referenced).any() and np.isfinite(nh).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_volume_to_cleaned_mesh_to_file(hip_device, tmp_path):
    from luciddreamer_amd import mesh, tsdf
    ref = MC.blobs_field()
    vol = tsdf.TSDFVolume(ref.origin.tolist(), float(ref.s), ref.dims, float(ref.trunc), hip_device)
    vol.tsdf.copy_(torch.from_numpy(ref.tsdf))
    vol.weight.copy_(torch.from_numpy(ref.weight))
    vol.color.copy_(torch.from_numpy(ref.color))
    V, C, F = vol.extract_mesh(1.0)
    want_V, want_C, want_F = MC.field_mesh("blobs")
    _same_bits("extracted faces", F, want_F)
    _same_bits("extracted vertices", V, want_V)
    V2, C2, F2, N2 = mesh.post_process(V, C, F, keep_largest=2, min_faces=50)
    wV, wC, wF, wN = MR.post_process(want_V, want_C, want_F, keep_largest=2, min_faces=50)
    assert len(wF) == 7916 - 52                                      # the three largest blobs without their faces of zero area
    _same_bits("faces", F2, wF)
    _same_bits("vertices", V2, wV)
    _same_bits("colors", C2, wC)
    _same_bits("normals", N2, wN)
    path = str(tmp_path / "blobs.ply")
    tsdf.save_mesh_ply(path, V2, C2, F2, normals=N2)
    xyz, nrm, rgb, idx = read_ply(path)
    _same_bits("xyz", xyz.copy(), wV)
    _same_bits("nxyz", nrm.copy(), wN)
    assert np.array_equal(idx, wF)
    assert np.array_equal(rgb, np.rint(np.clip(wC, 0, 1) * 255.0).astype(np.uint8))
    # without normals: the file the writer wrote before it took them
    from tests.test_mesh_cpu import _earlier_writer
    plain, earlier = str(tmp_path / "plain.ply"), str(tmp_path / "earlier.ply")
    tsdf.save_mesh_ply(plain, V2, C2, F2)
    _earlier_writer(earlier, wV, wC, wF)
    assert open(plain, "rb").read() == open(earlier, "rb").read()


# ---- hand-off -------------------------------------------------------------------------------------------------------------------
def test_hand_off(hip_device):
    from luciddreamer_amd import mesh
    v, c, f = MC.mesh("blobs")
    V, F = _dev(v, hip_device), _dev(f, hip_device)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh.vertex_normals(V.cpu(), F)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh.filter_clusters(V, F.cpu())
    with pytest.raises(TypeError, match="float32"):
        mesh.vertex_normals(V.double(), F)
    with pytest.raises(TypeError, match="int32"):
        mesh.vertex_normals(V, F.long())
    with pytest.raises(TypeError, match="int32"):
        mesh.connected_components(F.long(), len(v))
    with pytest.raises(TypeError, match="float32"):
        mesh.filter_clusters(V, F, colors=V.half())
    with pytest.raises(ValueError, match=r"\[n,3\]"):
        mesh.vertex_normals(V.reshape(-1), F)
    with pytest.raises(ValueError, match=r"\[n,3\]"):
        mesh.connected_components(F.reshape(-1, 2)[: len(f)], len(v))
    with pytest.raises(ValueError, match="colors must be"):
        mesh.filter_clusters(V, F, colors=V[:-1])
    with pytest.raises(ValueError, match="n_vertices"):
        mesh.connected_components(F, -1)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="is on"):
            mesh.vertex_normals(V, F.to("cuda:1"))


def test_misaligned_and_strided_inputs_are_converted(hip_device):
    from luciddreamer_amd import mesh
    v, c, f = MC.mesh("blobs")
    flat = torch.zeros(f.size + 1, dtype=torch.int32, device=hip_device)
    F = flat[1:].view(f.shape)                                                        # data_ptr() % 16 == 4
    F.copy_(torch.from_numpy(np.array(f)))
    assert F.data_ptr() % 16 == 4
    wide = torch.zeros(len(v), 5, dtype=torch.float32, device=hip_device)
    V = wide[:, 1:4]                                                                  # strided rows
    V.copy_(torch.from_numpy(np.array(v)))
    assert not V.is_contiguous()
    setting = (2, 1, True)
    want = MC.filter_reference("blobs", setting)
    V2, F2, vi, fi = mesh.filter_clusters(V, F, keep_largest=2, drop_degenerate=True, return_index=True)
    _same_bits("faces", F2, want["faces"])
    _same_bits("vertices", V2, want["vertices"])
    _same_bits("vertex_index", vi, want["vertex_index"])
    _same_bits("normals", mesh.vertex_normals(V, F), MC.normals_reference("blobs"))
    got = mesh.connected_components(F, len(v))
    for n, g, w in zip(("face_labels", "vertex_labels", "labels", "counts"), got, MC.components_reference("blobs")):
        _same_bits(n, g, w)
