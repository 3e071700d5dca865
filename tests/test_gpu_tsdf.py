"""TSDF fusion and mesh extraction on the device against the numpy restatement (tests/tsdf_ref.py), bit for bit: tsdf, weight,
colour, vertices, vertex colours and faces; the topology checks again on the device's own meshes; fuse_views against rendering
and integrating by hand; the PLY file through a minimal reader."""
import numpy as np
import pytest
import torch

from tests import posed_cases
from tests import tsdf_cases as TC
from tests import tsdf_ref as TR

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


def _device_volume(ref, dev):
    """A TSDFVolume with the restatement's lattice and a copy of its tensors."""
    from luciddreamer_amd import tsdf
    vol = tsdf.TSDFVolume(ref.origin.tolist(), float(ref.s), ref.dims, float(ref.trunc), dev, max_weight=float(ref.max_weight))
    vol.tsdf.copy_(torch.from_numpy(ref.tsdf))
    vol.weight.copy_(torch.from_numpy(ref.weight))
    vol.color.copy_(torch.from_numpy(ref.color))
    return vol


def _integrate(vol, variant, dev, one_by_one=False):
    with_color, with_pw, depth_max, _ = TC.INT_VARIANTS[variant]
    a = TC.integrate_inputs()
    t = lambda x: torch.from_numpy(np.array(x)).to(dev)
    depths = t(a["depths"])
    colors = t(a["colors"]) if with_color else None
    pw = t(a["pixel_weights"]) if with_pw else None
    if not one_by_one:
        return vol.integrate_batch(depths, a["K"], a["Rs"], a["Ts"], colors=colors, pixel_weights=pw, depth_max=depth_max)
    for f in range(TC.INT_F):
        vol.integrate(depths[f], a["K"], a["Rs"][f], a["Ts"][f], color=None if colors is None else colors[f],
                      pixel_weight=None if pw is None else pw[f], depth_max=depth_max)
    return vol


# ---- integrate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(TC.INT_VARIANTS))
def test_integrate_equals_the_restatement(hip_device, variant):
    ref, touched = TC.integrate_reference(variant)
    vol = _device_volume(TC.new_int_volume(TC.INT_VARIANTS[variant][3]), hip_device)
    # untouched voxels must not be written: give them a pattern the kernel would have to reproduce
    mark = np.float32(0.625)
    vol.tsdf.fill_(float(mark))
    vol.tsdf[torch.from_numpy(touched).to(hip_device)] = 1.0
    _integrate(vol, variant, hip_device)
    got_touched = (vol.weight > 0).cpu().numpy()
    assert np.array_equal(got_touched, touched)                       # the set of touched voxels is exact
    want_tsdf = np.where(touched, ref.tsdf, mark)
    _same_bits("tsdf", vol.tsdf, want_tsdf)
    _same_bits("weight", vol.weight, ref.weight)
    _same_bits("color", vol.color, ref.color)


def test_integrate_twice_gives_identical_bits_and_batch_equals_one_by_one(hip_device):
    runs = []
    for one_by_one in (False, False, True):
        vol = _device_volume(TC.new_int_volume(TC.INT_VARIANTS["limits"][3]), hip_device)
        _integrate(vol, "limits", hip_device, one_by_one=one_by_one)
        runs.append([t.cpu().numpy() for t in (vol.tsdf, vol.weight, vol.color)])
    for name, a, b, c in zip(("tsdf", "weight", "color"), *runs):
        _same_bits(name + " (second run)", b, a)
        _same_bits(name + " (one by one)", c, a)


def test_misaligned_and_strided_inputs_are_converted(hip_device):
    a = TC.integrate_inputs()
    ref, _ = TC.integrate_reference("plain")
    vol = _device_volume(TC.new_int_volume(), hip_device)
    flat = torch.zeros(a["depths"].size + 1, dtype=torch.float32, device=hip_device)
    off = flat[1:].view(a["depths"].shape)                             # data_ptr() % 16 == 4
    off.copy_(torch.from_numpy(np.array(a["depths"])))
    assert off.data_ptr() % 16 != 0
    vol.integrate_batch(off, a["K"], a["Rs"], a["Ts"])
    _same_bits("tsdf", vol.tsdf, ref.tsdf)
    _same_bits("weight", vol.weight, ref.weight)
    with pytest.raises(TypeError, match="float32"):
        vol.integrate_batch(off.double(), a["K"], a["Rs"], a["Ts"])
    with pytest.raises(ValueError, match="color must be"):
        vol.integrate_batch(off, a["K"], a["Rs"], a["Ts"], colors=torch.zeros(TC.INT_F, TC.INT_H, TC.INT_W, device=hip_device))
    with pytest.raises(RuntimeError, match="HIP device"):
        vol.integrate_batch(off.cpu(), a["K"], a["Rs"], a["Ts"])


# ---- extract ---------------------------------------------------------------------------------------------------------------------
def _check_topology(name, V, F):
    if name in ("sphere", "sphere_zeroed", "wide"):
        assert TR.is_closed(F) and TR.euler(len(V), F) == 2
    elif name == "torus":
        assert TR.is_closed(F) and TR.euler(len(V), F) == 0
    elif name == "plane":
        assert V[:, 0].max() <= TC.PLANE_X_MAX and TR.euler(len(V), F) == 1
        assert all(n == 1 for n in TR.directed_edges(F).values())
    if name == "sphere":
        tri = V[F].astype(np.float64)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert ((n * (tri.mean(axis=1) - TC.SPHERE_C)).sum(axis=1) > 0).all()


@pytest.mark.parametrize("name", TC.FIELD_NAMES)
def test_extract_equals_the_restatement(hip_device, name):
    ref = TC.field(name)
    want_V, want_C, want_F = TC.field_mesh(name)
    vol = _device_volume(ref, hip_device)
    V, C, F = vol.extract_mesh(1.0)
    assert V.device == C.device == F.device == vol.tsdf.device
    assert V.dtype == torch.float32 and C.dtype == torch.float32 and F.dtype == torch.int32
    assert tuple(V.shape) == want_V.shape and tuple(F.shape) == want_F.shape          # n_vertices, n_faces
    _same_bits("faces", F, want_F)
    _same_bits("vertices", V, want_V)
    _same_bits("colors", C, want_C)
    if name == "empty":
        assert V.shape[0] == 0 and F.shape[0] == 0
        return
    Vh, Fh = V.cpu().numpy(), F.cpu().numpy()
    assert TR.all_referenced(len(Vh), Fh)                                             # every vertex is referenced
    _check_topology(name, Vh, Fh)
    V2, C2, F2 = vol.extract_mesh(1.0)                                                # and again: identical bits
    _same_bits("faces (second run)", F2, Fh)
    _same_bits("vertices (second run)", V2, Vh)


def test_min_weight_selects_the_cells(hip_device):
    ref = TC.field("thin")
    vol = _device_volume(ref, hip_device)
    for mw in (0.5, 2.5, 3.0):
        want_V, want_C, want_F = ref.extract(mw)
        V, C, F = vol.extract_mesh(mw)
        _same_bits(f"faces at {mw}", F, want_F)
        _same_bits(f"vertices at {mw}", V, want_V)
    assert want_F.shape[0] == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_six_views_of_a_sphere_give_the_restatements_mesh(hip_device):
    from luciddreamer_amd import tsdf
    a = TC.e2e_inputs()
    ref, (want_V, want_C, want_F) = TC.e2e_reference()
    assert TR.is_closed(want_F) and TR.euler(len(want_V), want_F) == 2                # the restatement's mesh is closed
    vol = tsdf.TSDFVolume(TC.E2E_ORIGIN, TC.E2E_S, TC.E2E_DIMS, TC.E2E_TRUNC, hip_device)
    t = lambda x: torch.from_numpy(np.array(x)).to(hip_device)
    vol.integrate_batch(t(a["depths"]), a["K"], a["Rs"], a["Ts"], colors=t(a["colors"]))
    _same_bits("tsdf", vol.tsdf, ref.tsdf)
    _same_bits("weight", vol.weight, ref.weight)
    _same_bits("color", vol.color, ref.color)
    V, C, F = vol.extract_mesh()
    _same_bits("faces", F, want_F)
    _same_bits("vertices", V, want_V)
    _same_bits("colors", C, want_C)
    vol.reset()
    V, C, F = vol.extract_mesh()
    assert V.shape[0] == 0 and F.shape[0] == 0 and float(vol.tsdf.min()) == 1.0 and float(vol.weight.max()) == 0.0


# ---- fuse_views ------------------------------------------------------------------------------------------------------------------
FUSE_POSES = [(0.0, 0.0, 0.0, (0.0, 0.0, 0.0)), (0.25, 0.05, 0.1, (-0.6, 0.1, 0.2)), (-0.2, -0.1, 0.0, (0.5, -0.2, 0.3))]


def _wall(dev):
    """A wall of opaque Gaussians in the plane z = 3."""
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    g = torch.linspace(-1.6, 1.6, 41)
    y, x = torch.meshgrid(g, g, indexing="ij")
    P = x.numel()
    means = torch.stack([x.reshape(-1), y.reshape(-1), torch.full((P,), 3.0)], dim=1)
    gen = torch.Generator().manual_seed(3)
    shs = torch.rand(P, 1, 3, generator=gen) * 2.0 - 0.5
    scales = torch.tensor([0.07, 0.07, 0.01]).repeat(P, 1)
    rot = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(P, 1)
    return GaussianCloud(means.to(dev), scales.to(dev), rot.to(dev), torch.full((P, 1), 0.995).to(dev), shs.to(dev),
                         active_sh_degree=0, requires_grad=False)


@pytest.mark.parametrize("mode", ["median", "expected"])
def test_fuse_views_equals_rendering_and_integrating_by_hand(hip_device, mode):
    from luciddreamer_amd import tsdf
    from luciddreamer_amd.gaussian_renderer import DEFAULT_OPT, render
    pc = _wall(hip_device)
    bg = torch.tensor([0.1, 0.2, 0.3], device=hip_device)
    views = [posed_cases.camera(p, 64, 64).to(hip_device) for p in FUSE_POSES]
    make = lambda: tsdf.TSDFVolume((-1.0, -1.0, 2.45), 0.1, (21, 20, 11), 0.3, hip_device)
    fused = tsdf.fuse_views(make(), views, pc, DEFAULT_OPT, bg, depth=mode, alpha_min=0.5)
    hand = make()
    with torch.no_grad():
        for view in views:
            out = render(view, pc, DEFAULT_OPT, bg, return_alpha=True, return_median=mode == "median")
            alpha = out["alpha"].reshape(64, 64)
            d = out["median_depth"].reshape(64, 64) if mode == "median" else out["depth"].reshape(64, 64) / alpha
            d = torch.where(alpha < 0.5, torch.zeros_like(d), d)
            hand.integrate(d, *tsdf.pinhole_of(view), color=out["render"].permute(1, 2, 0).contiguous())
    w = fused.weight.cpu().numpy()
    D = fused.tsdf.cpu().numpy()
    assert (w == 3).any() and (w == 0).any() and (D[w > 0] < 0).any() and (D[w > 0] > 0).any()
    for name in ("tsdf", "weight", "color"):
        _same_bits(name, getattr(fused, name), getattr(hand, name).cpu().numpy())
    # the fused wall is where the Gaussians are: the zero crossing along z sits at 3 to within a voxel
    V, C, F = fused.extract_mesh(1.0)
    assert F.shape[0] > 0 and float((V[:, 2] - 3.0).abs().max()) < 0.1


# ---- the file --------------------------------------------------------------------------------------------------------------------
def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"],
                     ["list", "uchar", "int", "vertex_indices"]]
    v = np.frombuffer(body, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]), count=nv)
    f = np.frombuffer(body, dtype=np.dtype([("n", "u1"), ("idx", "<i4", 3)]), count=nf, offset=nv * 15)
    assert len(body) == nv * 15 + nf * 13 and (f["n"] == 3).all()
    return v["xyz"], v["rgb"], f["idx"]


def test_save_mesh_ply_round_trip(hip_device, tmp_path):
    from luciddreamer_amd import tsdf
    vol = _device_volume(TC.field("sphere"), hip_device)
    V, C, F = vol.extract_mesh()
    path = str(tmp_path / "sphere.ply")
    tsdf.save_mesh_ply(path, V, C, F)
    xyz, rgb, idx = _read_ply(path)
    _same_bits("xyz", xyz.copy(), V.cpu().numpy())
    assert np.array_equal(idx, F.cpu().numpy())
    assert np.array_equal(rgb, np.rint(np.clip(C.cpu().numpy(), 0, 1) * 255.0).astype(np.uint8))
    assert TR.is_closed(idx) and TR.euler(len(xyz), idx) == 2
