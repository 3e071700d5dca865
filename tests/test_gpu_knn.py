"""GPU: distCUDA2 (csrc/knn.hip, csrc/binning.hip, simple_knn/_C.py) on the clouds of tests/knn_cases.py -- real scene
statistics, degenerate inputs, every size around the box / tile / wave boundaries -- against the brute-force oracles, per row:
12u against float32 (oracle_dist2), 8u against float64 (oracle_dist2_f64); tests/test_knn_oracle_cpu.py derives the factors.
Beyond the result: the Morton stage read back through lr_dist2_workspace_layout (a wrong or unstable sort still gives exact
results, only slower, so only the stage shows it), a dirty workspace, repeatability, input handling, and the radix sort's
multi-tile loop (P > 2 097 152), which no smaller cloud reaches.

Largest cloud 5 M points (workspace about 250 MB); the `offset` clouds, on which pruning does nothing, stay at 20 000."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import knn_cases as kc

pytestmark = pytest.mark.gpu

BOX = 256                        # csrc/knn.hip: points per box
TILE = 2048                      # csrc/common.h SORT_TILE; up to 1024 blocks own one tile each: P <= 2 097 152
N_SAMPLE = 4096                  # seeded random rows of a large cloud that go to the CPU oracle (plus 64 smallest, 64 largest)


def _lib():
    from luciddreamer_amd import _lib as lib_mod
    return lib_mod.lib()


def _dist(pts, dev):
    from simple_knn._C import distCUDA2
    return distCUDA2(torch.from_numpy(pts).to(dev)).cpu().numpy()


def _raw(pts_dev, ws_fill=None):
    """lr_dist2 called directly: out pre-filled with NaN (a row nobody writes stays NaN), the workspace optionally pre-filled with
    a byte.  Returns (out, workspace) as device tensors, after a synchronise."""
    L = _lib()
    P = int(pts_dev.shape[0])
    assert pts_dev.is_contiguous() and pts_dev.dtype == torch.float32
    ws = torch.empty((L.lr_dist2_workspace_bytes(P),), dtype=torch.uint8, device=pts_dev.device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    out = torch.full((P,), float("nan"), dtype=torch.float32, device=pts_dev.device)
    rc = L.lr_dist2(P, pts_dev.data_ptr(), out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(pts_dev.device).cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize(pts_dev.device)
    return out, ws


def _stage(P, ws):
    """(keys, order, sorted_pts, boxes) as lr_dist2 left them in the workspace."""
    off = (ctypes.c_size_t * 4)()
    assert _lib().lr_dist2_workspace_layout(P, off) == 0
    nbox = (P + BOX - 1) // BOX
    w = ws.cpu().numpy()
    assert max(off[0], off[1]) + 4 * P <= w.size and off[2] + 16 * P <= w.size and off[3] + 32 * nbox <= w.size
    assert len({off[0], off[1], off[2], off[3]}) == 4 and all(o % 16 == 0 for o in off)
    keys = w[off[0]:off[0] + 4 * P].view(np.uint32)
    order = w[off[1]:off[1] + 4 * P].view(np.uint32)
    sorted_pts = w[off[2]:off[2] + 16 * P].view(np.uint32).reshape(P, 4)
    boxes = w[off[3]:off[3] + 32 * nbox].view(np.float32).reshape(nbox, 8)
    return keys, order, sorted_pts, boxes


def _spread(x):
    x = x.astype(np.uint32)
    x = (x | (x << 16)) & 0x030000FF
    x = (x | (x << 8)) & 0x0300F00F
    x = (x | (x << 4)) & 0x030C30C3
    x = (x | (x << 2)) & 0x09249249
    return x


def _host_morton(pts):
    """The 30-bit Morton code of every point, in float32 as k_morton forms it: the scene box is seeded with the origin (as the
    reference's reduction is), t = (v - min) / extent (0 where the extent is 0), clamped, cell = trunc(t * 1023)."""
    mn = np.minimum(pts.min(axis=0), np.float32(0.0)).astype(np.float32)
    mx = np.maximum(pts.max(axis=0), np.float32(0.0)).astype(np.float32)
    ext = (mx - mn).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ext > 0, ((pts - mn).astype(np.float32) / ext).astype(np.float32), np.float32(0.0)).astype(np.float32)
    t = np.minimum(np.maximum(t, np.float32(0.0)), np.float32(1.0))
    cell = (t * np.float32(1023.0)).astype(np.float32).astype(np.uint32)
    return _spread(cell[:, 0]) | (_spread(cell[:, 1]) << 1) | (_spread(cell[:, 2]) << 2)


@functools.lru_cache(maxsize=4)
def _large_points(kind, P):
    return kc.surface(P, 7) if kind == "surface" else kc.synthetic_cloud(kind, P, 5)


# ---------------------------------------------------------------------------------------------------------------------------
# results
# ---------------------------------------------------------------------------------------------------------------------------
def test_knn_parity_and_properties(hip_device):
    from simple_knn._C import distCUDA2
    from luciddreamer_amd import synthetic
    pts = synthetic.make_cloud(20_000, "box", 4)["means3D"]
    got = distCUDA2(pts.to(hip_device)).cpu().numpy()
    kc.assert_rows(got, oracle.dist2(pts.numpy()), kc.BAR_F32, "box 20000")
    # tiny and degenerate inputs
    for P in (1, 2, 3, 4, 257):
        p = torch.rand(P, 3, generator=torch.Generator().manual_seed(P))
        a = distCUDA2(p.to(hip_device)).cpu().numpy()
        kc.assert_rows(a, oracle.dist2(p.numpy()), kc.BAR_F32, f"uniform {P}")
    # large: permutation equivariance (result is written at the original index)
    big = synthetic.make_cloud(300_000, "band", 5)["means3D"]
    perm = torch.randperm(300_000, generator=torch.Generator().manual_seed(0))
    d1 = distCUDA2(big.to(hip_device)).cpu()
    d2 = distCUDA2(big[perm].contiguous().to(hip_device)).cpu()
    assert torch.equal(d1[perm], d2)
    assert float(d1.min()) > 0


@pytest.mark.parametrize("case", kc.CASES, ids=kc.case_ids())
def test_parity_on_the_table(hip_device, case):
    """Every row of every case within 12u of oracle_dist2 and 8u of the float64 reference; rows with three coincident others
    exactly 0.0, the unit lattice exactly 1.0, fewer than 4 points exactly the oracle's FLT_MAX-slot values."""
    pts = case.make(case.P)
    P = pts.shape[0]
    got = _dist(pts, hip_device)
    assert got.shape == (P,) and got.dtype == np.float32
    ref32, ref64 = oracle.dist2(pts), oracle.dist2_f64(pts)
    r32, r64 = kc.row_ratio(got, ref32), kc.row_ratio(got, ref64)
    fin = np.isfinite(ref32) & np.isfinite(got)
    old = float(np.abs(got[fin] - ref32[fin]).max() / ref32[fin].max()) if fin.any() and ref32[fin].max() > 0 else 0.0
    print(f"knn-gpu-ratio {case.name} P={P} f32={r32.max():.3f}u f64={r64.max():.3f}u max|a-b|/b.max()={old:.2e}")
    kc.assert_rows(got, ref32, kc.BAR_F32, f"{case.name} against oracle_dist2")
    kc.assert_rows(got, ref64, kc.BAR_F64, f"{case.name} against oracle_dist2_f64")
    if P < 4:
        assert np.array_equal(got.view(np.uint32), ref32.view(np.uint32)), (got, ref32)
    assert np.all(got[kc.zero_rows(pts)] == 0.0)
    if case.exact is not None:
        assert np.all(got == np.float32(case.exact)), (case.name, np.unique(got)[:8])


LARGE = [("surface", 2_097_152), ("surface", 2_097_153), ("surface", 5_000_000),
         ("band", 2_097_152), ("band", 2_097_153), ("band", 5_000_000)]


@pytest.mark.parametrize("kind,P", LARGE, ids=[f"{k}_{p}" for k, p in LARGE])
def test_large_clouds(hip_device, kind, P):
    """P = 2 097 152 is the last size at which every block of the radix scatter owns one 2048-key tile; at 2 097 153 a block owns
    two and carries its running digit offsets from tile to tile; 5 M is three tiles.  All rows: written (no NaN left of the pre-fill), finite, >= 0, and what distCUDA2
    returns.  Sampled rows (4 096 seeded, the 64 smallest and the 64 largest results) against oracle_dist2_subset, 12u."""
    pts = _large_points(kind, P)
    dev = torch.from_numpy(pts).to(hip_device)
    out, _ = _raw(dev)
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} rows never written"
    assert np.isfinite(got).all() and (got >= 0).all()
    from simple_knn._C import distCUDA2
    assert np.array_equal(distCUDA2(dev).cpu().numpy().view(np.uint32), got.view(np.uint32))
    rng = np.random.Generator(np.random.PCG64(P))
    part = np.argpartition(got, (64, P - 65))
    rows = np.concatenate([rng.choice(P, size=N_SAMPLE, replace=False), part[:64], part[-64:]]).astype(np.int32)
    ref = oracle.dist2_subset(pts, rows)
    worst = kc.assert_rows(got[rows], ref, kc.BAR_F32, f"{kind} {P} sampled rows")
    print(f"knn-gpu-large {kind} P={P} rows={rows.size} f32={worst:.3f}u")


@pytest.mark.parametrize("kind", ["surface", "band"])
def test_large_two_tile_cloud_all_rows_against_kdtree(hip_device, kind):
    """The extra of the large case: all 2 097 153 rows against a float64 k = 4 query (needs scipy; the sampled check does not)."""
    spatial = pytest.importorskip("scipy.spatial")
    P = 2_097_153
    pts = _large_points(kind, P)
    got = _dist(pts, hip_device)
    p64 = pts.astype(np.float64)
    d, _ = spatial.cKDTree(p64).query(p64, k=4, workers=-1)
    ref = (d[:, 1:] ** 2).sum(axis=1) / 3.0
    worst = kc.assert_rows(got, ref, kc.BAR_F64, f"{kind} {P} all rows against cKDTree")
    print(f"knn-gpu-kdtree {kind} P={P} f64={worst:.3f}u")


# ---------------------------------------------------------------------------------------------------------------------------
# the Morton stage
# ---------------------------------------------------------------------------------------------------------------------------
def _stage_points(name):
    if name == "box_70000":
        return kc.synthetic_cloud("box", 70_000, 11)
    if name == "surface_2097153":
        return _large_points("surface", 2_097_153)
    return kc.BY_NAME[name].make(kc.BY_NAME[name].P)


@pytest.mark.parametrize("name", ["box_70000", "duplicates", "offset_positive", "all_identical", "surface_2097153"])
def test_morton_stage(hip_device, name):
    """What lr_dist2 leaves in its workspace: the order is a permutation; keys are non-decreasing; equal keys keep increasing
    original index (the sort is stable and its first pass numbers the points itself); sorted_pts[i] is input row order[i] bit
    for bit, with the index in .w; every key is the Morton code of its point, recomputed on the host in float32 (exactly: the
    build rounds the division correctly and nothing in the code can contract); every box is the min/max of its <= 256 points,
    the last, partial box included."""
    pts = _stage_points(name)
    P = pts.shape[0]
    out, ws = _raw(torch.from_numpy(pts).to(hip_device), ws_fill=0xFF)
    keys, order, sorted_pts, boxes = _stage(P, ws)
    assert np.array_equal(np.sort(order), np.arange(P, dtype=np.uint32)), "order is not a permutation of 0..P-1"
    assert np.all(keys[1:] >= keys[:-1]), f"{int((keys[1:] < keys[:-1]).sum())} descents in the sorted keys"
    ties = keys[1:] == keys[:-1]
    assert np.all(order[1:][ties] > order[:-1][ties]), "equal keys out of input order: the sort is not stable"
    assert np.array_equal(sorted_pts[:, :3], pts.view(np.uint32)[order])
    assert np.array_equal(sorted_pts[:, 3], order)
    want = _host_morton(pts)[order]
    n_off = int((keys != want).sum())
    print(f"knn-gpu-stage {name} P={P} distinct keys {np.unique(keys).size} keys differing from the host's {n_off}")
    assert n_off == 0
    assert keys.max() < (1 << 30)
    xyz = sorted_pts[:, :3].view(np.float32)
    starts = np.arange(0, P, BOX)
    assert np.array_equal(boxes[:, 0:3], np.minimum.reduceat(xyz, starts, axis=0))
    assert np.array_equal(boxes[:, 4:7], np.maximum.reduceat(xyz, starts, axis=0))
    if name == "all_identical":
        assert np.unique(keys).size == 1 and np.array_equal(order, np.arange(P, dtype=np.uint32))
    assert not np.isnan(out.cpu().numpy()).any()


@pytest.mark.parametrize("name", ["box_70000", "duplicates", "box_257", "surface_2049", "all_identical"])
def test_dirty_workspace(hip_device, name):
    """Every word of the workspace that is read was written first: 0x00-filled and 0xFF-filled workspaces give the same bits,
    and so does distCUDA2's torch.empty.  The result alone cannot show it (pruning is conservative for any scene box and any
    order, so a scene box reduced from garbage still gives exact distances): the sorted keys, the order, the sorted points and
    the boxes must be the same bits too, and the keys those of the host's origin-seeded scene box."""
    pts = _stage_points(name)
    P = pts.shape[0]
    dev = torch.from_numpy(pts).to(hip_device)
    a, wa = _raw(dev, ws_fill=0x00)
    b, wb = _raw(dev, ws_fill=0xFF)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert not np.isnan(a).any() and not np.isnan(b).any()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), _dist(pts, hip_device).view(np.uint32))
    sa, sb = _stage(P, wa), _stage(P, wb)
    for x, y, what in zip(sa[:3], sb[:3], ("keys", "order", "sorted_pts")):
        assert np.array_equal(x, y), what
    assert np.array_equal(sa[3][:, (0, 1, 2, 4, 5, 6)].view(np.uint32), sb[3][:, (0, 1, 2, 4, 5, 6)].view(np.uint32)), "boxes"
    assert np.array_equal(sa[0], _host_morton(pts)[sa[1]]), "keys of a scene box that was not seeded with the origin"


def test_repeatable(hip_device):
    from simple_knn._C import distCUDA2
    dev = torch.from_numpy(kc.surface(300_000, 3)).to(hip_device)
    first = distCUDA2(dev)
    for _ in range(4):
        assert torch.equal(distCUDA2(dev).view(torch.int32), first.view(torch.int32))


@pytest.mark.parametrize("name", ["band", "surface", "duplicates"])
def test_permutation_equivariance(hip_device, name):
    pts = {"band": lambda: kc.synthetic_cloud("band", 300_000, 5), "surface": lambda: kc.surface(196_608, 2),
           "duplicates": lambda: kc.duplicates(30_000, 1)}[name]()
    P = pts.shape[0]
    perm = np.random.Generator(np.random.PCG64(0)).permutation(P)
    d1 = _dist(pts, hip_device)
    d2 = _dist(np.ascontiguousarray(pts[perm]), hip_device)
    assert np.array_equal(d1[perm].view(np.uint32), d2.view(np.uint32))
    if name != "duplicates":
        assert d1.min() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# simple_knn/_C.py
# ---------------------------------------------------------------------------------------------------------------------------
def test_input_handling(hip_device):
    from simple_knn._C import distCUDA2
    pts = kc.surface(10_000, 5)
    P = pts.shape[0]
    want = _dist(pts, hip_device)
    kc.assert_rows(want, oracle.dist2(pts), kc.BAR_F32, "surface 10000")

    def same(t):
        keep = t.clone()
        got = distCUDA2(t)
        assert got.shape == (P,) and got.dtype == torch.float32 and got.device == t.device
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert torch.equal(t, keep), "the input was modified"

    p = torch.from_numpy(pts).to(hip_device)
    same(p)
    pts4 = torch.cat([p, torch.full((P, 1), 7.0, device=hip_device)], dim=1)
    v = pts4[:, :3]                                                       # row stride 4: not contiguous
    assert not v.is_contiguous()
    same(v)
    assert torch.all(pts4[:, 3] == 7.0)
    base = torch.full((P + 5, 3), -3.0, device=hip_device)
    base[5:] = p
    off = base[5:]                                                        # contiguous, storage offset 15 floats
    assert off.is_contiguous() and off.storage_offset() == 15
    same(off)
    assert torch.all(base[:5] == -3.0)
    same(p.t().contiguous().t())                                          # column-major view

    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        q = p * 1.0                                                       # produced on the side stream
        twice = distCUDA2(q) * 2.0                                        # ... and used on it
    side.synchronize()
    assert np.array_equal(twice.cpu().numpy(), want * np.float32(2.0))

    with pytest.raises(RuntimeError, match="float32"):
        distCUDA2(p.double())
    with pytest.raises(RuntimeError, match="HIP device"):
        distCUDA2(torch.from_numpy(pts))
    empty = distCUDA2(torch.empty((0, 3), device=hip_device))
    assert empty.shape == (0,) and empty.dtype == torch.float32 and empty.device.type == "cuda"


def test_workspace_layout_query():
    """Host function: no device needed to ask, but the library only loads beside the HIP runtime."""
    L = _lib()
    off = (ctypes.c_size_t * 4)()
    for P in (0, 1, 256, 257, 2_097_153, 5_000_000):
        assert L.lr_dist2_workspace_layout(P, off) == 0
        nbox = (max(P, 1) + BOX - 1) // BOX
        total = L.lr_dist2_workspace_bytes(P)
        assert max(off[0], off[1]) + 4 * P <= total and off[2] + 16 * P <= total and off[3] + 32 * nbox <= total
    assert L.lr_dist2_workspace_layout(-1, off) < 0
    assert L.lr_dist2_workspace_layout(10, None) < 0
