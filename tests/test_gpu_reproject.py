"""Point-cloud reprojection on the GPU (csrc/reproject.hip through luciddreamer_amd.reproject) against the numpy restatement
(tests/reproject_ref.py).  Every output is compared for exact equality: integers, and floats formed from integer sums by one
documented float64 expression.  The shapes are the smallest at which each path can still go wrong: more than one workgroup,
sizes that are no multiple of the tile or of the workgroup, more frames than one per-point launch carries."""
import os

import numpy as np
import pytest
import torch

from tests import reproject_ref as RR

pytestmark = pytest.mark.gpu

FIELDS = ("image", "image_u8", "mask", "dil", "border", "depth", "valid", "pix")


def _pose(rng):
    a, b, c = rng.uniform(-0.08, 0.08, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rx @ Ry @ Rz, rng.uniform(-0.1, 0.1, (3, 1))


def _intrinsics(H, W):
    return np.array([[0.9 * W, 0, W / 2.0], [0, 0.9 * W, H / 2.0], [0, 0, 1]], dtype=np.float64)


def _cloud(seed, N, H, W, cover=0.68, behind=0.02):
    """Two depth layers (the far one 2x the near one: behind it by far more than the z tolerance) over `cover` of the view, a
    sparse sprinkle over the rest, points off screen and behind the camera.  X is [3,N] float32, as the reference holds it."""
    rng = np.random.default_rng(seed)
    K = _intrinsics(H, W)
    R, T = _pose(rng)
    n_sparse = min(25, N // 4)
    u = np.concatenate([rng.uniform(-6, cover * W, N - n_sparse), rng.uniform(cover * W, W + 4, n_sparse)])
    v = rng.uniform(-6, H + 5, N)
    z = np.where(rng.random(N) < 0.5, rng.uniform(2.8, 3.2, N), rng.uniform(5.5, 6.5, N))
    z[rng.random(N) < behind] *= -1
    cam = np.linalg.inv(K) @ np.stack([u * z, v * z, z])
    X = np.ascontiguousarray((np.linalg.inv(R) @ (cam - T)).astype(np.float32))
    C = rng.random((N, 3)).astype(np.float32)
    return X, C, K, R, T


def _device_frame(dev, X, C, K, R, T, H, W, **kw):
    from luciddreamer_amd import reproject
    f = reproject.project(torch.from_numpy(X).to(dev), torch.from_numpy(C).to(dev), K, R, T, H, W, **kw)
    return dict(image=f.image, image_u8=f.image_u8, mask=f.mask, dil=f.dilated, border=f.border, depth=f.depth, valid=f.valid,
                pix=f.pix)


def _assert_equal(got, want, what=""):
    for k in FIELDS:
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].dtype, want[k].shape)
        assert np.array_equal(g, want[k]), (what, k, int((g != want[k]).sum()))


_REF = {}


def _ref(key, X, C, K, R, T, H, W, **kw):
    """The restatement of a case, computed once and shared."""
    if key not in _REF:
        _REF[key] = RR.project(X, C, K, R, T, H, W, **kw)
    return _REF[key]


# ---- a: random clouds in two depth layers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W, N", [(48, 64, 3 * 48 * 64), (37, 53, 3 * 37 * 53), (48, 64, 3 * 48 * 64 - 1)])
def test_a_random_cloud_in_two_layers(hip_device, H, W, N):
    X, C, K, R, T = _cloud(H * 1000 + N, N, H, W)
    want = _ref(("a", H, W, N), X, C, K, R, T, H, W)
    assert 0 < want["mask"].sum() < H * W and want["border"].any() and 0 < want["valid"].sum() < N
    assert (want["S"] == 0)[want["mask"] == 1].any()                          # the window fill runs
    loose = RR.project(X, C, K, R, T, H, W, z_tolerance=10.0)
    assert not np.array_equal(loose["image"], want["image"])                   # the z test decides pixels of this cloud
    _assert_equal(_device_frame(hip_device, X, C, K, R, T, H, W), want, "[3,N]")
    _assert_equal(_device_frame(hip_device, np.ascontiguousarray(X.T), C, K, R, T, H, W), want, "[N,3]")
    _assert_equal(_device_frame(hip_device, X, C, K, R, T, H, W, z_tolerance=10.0), loose, "z_tolerance 10")


@pytest.mark.parametrize("name", ["a", "b", "grid"])
def test_a_fixture_clouds_give_the_reference_masks(hip_device, name):
    """The device against what the reference's own host code and scipy made of the fixture clouds (tests/golden/
    ref_reproject_fixtures.npz): valid_idx, rounded coordinates, round_mask2, mask2, mask_hf and border_valid_idx, bit for bit."""
    from luciddreamer_amd import reproject
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_reproject_fixtures.npz"))
    H, W = (int(v) for v in fx[f"{name}_HW"])
    f = reproject.project(torch.from_numpy(fx[f"{name}_X"]).to(hip_device), torch.from_numpy(fx[f"{name}_C"]).to(hip_device),
                          fx[f"{name}_K"], fx[f"{name}_R"], fx[f"{name}_T"], H, W)
    valid_idx = f.valid.nonzero()[:, 0]
    pix = f.pix[valid_idx].long()
    assert np.array_equal(valid_idx.cpu().numpy(), fx[f"{name}_valid_idx"])
    assert np.array_equal(torch.stack([pix % W, pix // W]).cpu().numpy(), fx[f"{name}_round_coord"])
    assert np.array_equal(f.dilated.cpu().numpy(), fx[f"{name}_round_mask"])
    assert np.array_equal(f.mask.cpu().numpy(), fx[f"{name}_mask2"])
    assert np.array_equal(f.border.cpu().numpy(), fx[f"{name}_mask_hf"])
    border_valid_idx = f.border.flatten()[pix].nonzero()[:, 0]
    assert np.array_equal(border_valid_idx.cpu().numpy(), fx[f"{name}_border_valid_idx"])


# ---- b: exact ties and the closed validity bounds -------------------------------------------------------------------------------
def test_b_ties_round_half_to_even_and_bounds_are_closed(hip_device):
    H, W = 9, 12
    us = np.array([0.0, 0.5, 1.5, 2.5, 3.5, W - 1.5, W - 1.0, W - 0.5, -0.5], dtype=np.float32)
    vs = np.array([0.0, 0.5, 1.5, 2.5, H - 1.5, H - 1.0, H - 0.5, -0.5], dtype=np.float32)
    uu, vv = np.meshgrid(us, vs, indexing="xy")
    X = np.ascontiguousarray(np.stack([uu.ravel(), vv.ravel(), np.ones(uu.size, dtype=np.float32)]))
    C = np.random.default_rng(3).random((X.shape[1], 3)).astype(np.float32)
    K, R, T = np.eye(3), np.eye(3), np.zeros((3, 1))
    want = _ref("b", X, C, K, R, T, H, W)
    # what exact arithmetic demands, spelled out
    ok_u = {0.0: 0, 0.5: 0, 1.5: 2, 2.5: 2, 3.5: 4, W - 1.5: W - 2 if (W - 2) % 2 == 0 else W - 1, W - 1.0: W - 1}
    ok_v = {0.0: 0, 0.5: 0, 1.5: 2, 2.5: 2, H - 1.5: H - 2 if (H - 2) % 2 == 0 else H - 1, H - 1.0: H - 1}
    for i in range(X.shape[1]):
        u, v = float(X[0, i]), float(X[1, i])
        if u in ok_u and v in ok_v:
            assert want["valid"][i] == 1 and want["pix"][i] == ok_v[v] * W + ok_u[u], (u, v)
        else:
            assert want["valid"][i] == 0 and want["pix"][i] == -1, (u, v)
    _assert_equal(_device_frame(hip_device, X, C, K, R, T, H, W), want)


# ---- c: 20 000 points in one pixel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", ["one_cell", "four_cells"])
def test_c_many_points_in_one_pixel(hip_device, spread):
    H, W, N = 16, 24, 20_000
    rng = np.random.default_rng(11)
    lo, hi = (0.05, 0.45) if spread == "one_cell" else (-0.45, 0.45)          # one bilinear cell (summed per wave) or four
    u = (10.0 + rng.uniform(lo, hi, N)).astype(np.float32)
    v = (7.0 + rng.uniform(lo, hi, N)).astype(np.float32)
    z = np.where(rng.random(N) < 0.9, 1.0, 1.0 + rng.uniform(0.0, 0.1, N)).astype(np.float32)     # some fail the 5 % z test
    X = np.ascontiguousarray(np.stack([u * z, v * z, z]).astype(np.float32))
    C = rng.random((N, 3)).astype(np.float32)
    C[:2000] = 1.0                                                            # full-scale terms: 65536 * 65535 each
    K, R, T = np.eye(3), np.eye(3), np.zeros((3, 1))
    want = _ref(("c", spread), X, C, K, R, T, H, W)
    assert want["valid"].all() and want["hit"].sum() == 1 and want["hit"][7, 10] == 1
    assert int(want["A"].max()) > 2 ** 32 and int(want["S"][7, 10]) > 2 ** 16
    _assert_equal(_device_frame(hip_device, X, C, K, R, T, H, W), want)


# ---- d, e: points that are all invalid ------------------------------------------------------------------------------------------
def test_d_invalid_points_write_nowhere(hip_device):
    from luciddreamer_amd import reproject
    H, W = 20, 30
    K, R, T = _intrinsics(H, W), np.eye(3), np.zeros((3, 1))
    nan, inf = float("nan"), float("inf")
    X = np.array([[0, 0, -2], [0.1, 0.1, -1e-3], [0, 0, 0], [5, 0, 2], [-5, 0, 2], [0, 5, 2], [0, -5, 2],       # behind, off screen
                  [nan, 0, 2], [0, nan, 2], [0, 0, nan], [nan, nan, nan], [inf, 0, 2], [0, 0, inf], [-inf, inf, 1]],
                 dtype=np.float32)
    X = np.ascontiguousarray(np.tile(X, (40, 1)))                             # 560 points: more than one workgroup
    C = np.ones((X.shape[0], 3), dtype=np.float32)
    want = _ref("d", X, C, K, R, T, H, W)
    assert not want["valid"].any() and (want["pix"] == -1).all()
    for k in ("image", "image_u8", "mask", "dil", "border", "depth"):
        assert not want[k].any(), k
    _assert_equal(_device_frame(hip_device, X, C, K, R, T, H, W), want)
    # e: no point at all
    empty = reproject.project(torch.zeros((0, 3), device=hip_device), torch.zeros((0, 3), device=hip_device), K, R, T, H, W)
    for k in ("image", "image_u8", "mask", "dilated", "border", "depth"):
        t = getattr(empty, k)
        assert t.shape[:2] == (H, W) and not t.any(), k
    assert empty.valid.numel() == 0 and empty.pix.numel() == 0


# ---- f: a sparse cloud ----------------------------------------------------------------------------------------------------------
def test_f_sparse_cloud_fills_windows_and_clamps_at_the_edge(hip_device):
    H, W, N = 37, 53, 40
    rng = np.random.default_rng(17)
    K, R, T = _intrinsics(H, W), np.eye(3), np.zeros((3, 1))
    u = rng.uniform(0, W - 1, N)
    v = rng.uniform(0, H - 1, N)
    u[:4], v[:4] = [0.2, W - 1.2, 0.3, W - 1.3], [0.2, 0.3, H - 1.2, H - 1.3]                 # the four corners
    u[4:12], v[4:12] = 20 + 3.0 * (np.arange(8) % 4), 15 + 3.0 * (np.arange(8) // 4)          # a cluster dense enough for `mask`
    z = rng.uniform(2, 3, N)
    X = np.ascontiguousarray((np.linalg.inv(K) @ np.stack([u * z, v * z, z])).astype(np.float32))
    C = rng.random((N, 3)).astype(np.float32)
    want = _ref("f", X, C, K, R, T, H, W)
    assert want["valid"].all() and want["mask"].any() and want["border"].any()
    assert want["dil"][0, 0] and want["dil"][H - 1, W - 1] and want["dil"][0, W - 1] and want["dil"][H - 1, 0]
    filled = (want["mask"] == 1) & (want["S"] == 0)
    assert filled.sum() > 10 and want["image"][filled].any()
    _assert_equal(_device_frame(hip_device, X, C, K, R, T, H, W), want)


# ---- g, h: batches and repeatability --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 9])                                         # 9: more frames than one per-point launch carries
def test_g_batch_equals_single_calls(hip_device, F):
    from luciddreamer_amd import reproject
    H, W, N = 37, 53, 3000
    X, C, K, _, _ = _cloud(23, N, H, W, cover=0.8)
    rng = np.random.default_rng(29)
    poses = [_pose(rng) for _ in range(F)]
    Xd, Cd = torch.from_numpy(X).to(hip_device), torch.from_numpy(C).to(hip_device)
    batch = reproject.project_batch(Xd, Cd, K, np.stack([r for r, _ in poses]), np.stack([t for _, t in poses]), H, W)
    assert batch.valid is None and batch.pix is None and batch.image.shape == (F, H, W, 3)
    distinct = set()
    for j, (R, T) in enumerate(poses):
        one = reproject.project(Xd, Cd, K, R, T, H, W)
        for k in ("image", "image_u8", "mask", "dilated", "border", "depth"):
            assert torch.equal(getattr(batch, k)[j], getattr(one, k)), (j, k)
        distinct.add(one.image_u8.cpu().numpy().tobytes())
        if j in (0, F - 1):
            want = _ref(("g", j, F), X, C, K, R, T, H, W)
            _assert_equal(dict(image=one.image, image_u8=one.image_u8, mask=one.mask, dil=one.dilated, border=one.border,
                               depth=one.depth, valid=one.valid, pix=one.pix), want, f"pose {j}")
    assert len(distinct) == F                                                  # the poses do differ


def test_h_two_runs_give_the_same_bits(hip_device):
    H, W, N = 48, 64, 3 * 48 * 64
    X, C, K, R, T = _cloud(H * 1000 + N, N, H, W)
    a = _device_frame(hip_device, X, C, K, R, T, H, W)
    b = _device_frame(hip_device, X, C, K, R, T, H, W)
    for k in FIELDS:
        assert torch.equal(a[k], b[k]), k


# ---- i: lift ------------------------------------------------------------------------------------------------------------------
def test_i_lift_equals_the_float64_restatement(hip_device):
    from luciddreamer_amd import reproject
    H, W = 37, 53
    rng = np.random.default_rng(31)
    K = _intrinsics(H, W)
    R, T = _pose(rng)
    depth = rng.uniform(0.5, 8.0, (H, W)).astype(np.float32)
    depth[3, 5], depth[10, 10] = 0.0, -1.0
    got = reproject.lift(torch.from_numpy(depth).to(hip_device), K, R, T).cpu().numpy()
    ref64 = RR.lift_f64(depth, K, R, T)
    ref32 = ref64.astype(np.float32)
    assert got.shape == (3, H * W) and got.dtype == np.float32
    # a float64 value half way between two float32 neighbours is the only place a correctly rounded conversion could be argued
    # about: count them (none on this depth map), and demand equality everywhere else
    up, down = np.nextafter(ref32, np.float32(np.inf)), np.nextafter(ref32, np.float32(-np.inf))
    on_boundary = (ref64 == (ref32.astype(np.float64) + up.astype(np.float64)) / 2) | \
                  (ref64 == (ref32.astype(np.float64) + down.astype(np.float64)) / 2)
    assert int(on_boundary.sum()) == 0
    differs = got != ref32
    assert not (differs & ~on_boundary).any(), int(differs.sum())
    assert (np.abs(got[differs].view(np.int32) - ref32[differs].view(np.int32)) <= 1).all()
    # and the round trip: the lifted points land on their own pixels at the same pose (interior pixels: float32 rounding of a
    # point of the outermost rows and columns may carry it across the closed bound)
    inner = np.zeros((H, W), dtype=bool)
    inner[1:-1, 1:-1] = True
    pos = ((depth > 0) & inner).reshape(-1)
    back = RR.project(got, np.zeros((H * W, 3), dtype=np.float32), K, R, T, H, W)
    assert back["valid"][pos].all() and np.array_equal(back["pix"][pos], np.arange(H * W, dtype=np.int32)[pos])


# ---- j: align_frames ----------------------------------------------------------------------------------------------------------
def _hemisphere(n, rng):
    poses = np.tile(np.eye(4)[None], (n, 1, 1))
    for j in range(1, n):
        poses[j, :3, :3], poses[j, :3, 3:] = _pose(rng)
    return poses


def test_j_align_frames(hip_device):
    from PIL import Image
    from luciddreamer_amd import reproject
    H, W, N = 37, 53, 3000
    X, C, K, R0, T0 = _cloud(41, N, H, W, cover=0.9, behind=0.0)
    rng = np.random.default_rng(43)
    render = np.tile(np.eye(4)[None], (2, 1, 1))
    render[0, :3, :3], render[0, :3, 3:] = R0, T0
    render[1, :3, :3], render[1, :3, 3:] = _pose(rng)
    inner = _hemisphere(5, rng)
    Xd, Cd = torch.from_numpy(X).to(hip_device), torch.from_numpy(C).to(hip_device)
    data = reproject.align_frames(Xd, Cd, K, render, inner, H, W, 0.9)
    assert set(data) == {"camera_angle_x", "W", "H", "pcd_points", "pcd_colors", "frames"}
    assert data["camera_angle_x"] == 0.9 and data["W"] == W and data["H"] == H
    assert np.array_equal(data["pcd_points"], X) and np.array_equal(data["pcd_colors"], C)
    assert len(data["frames"]) == 10
    tensors = reproject.align_frames(Xd, Cd, K, render, inner, H, W, 0.9, as_tensors=True)
    k = 0
    for i in range(2):
        for j in range(5):
            Rw2j, Tw2j = RR.compose_pose(inner[j, :3, :3], inner[j, :3, 3:4], render[i, :3, :3], render[i, :3, 3:4])
            f = data["frames"][k]
            assert set(f) == {"image", "transform_matrix"} and isinstance(f["image"], Image.Image)
            assert f["transform_matrix"] == RR.pc2w(Rw2j, Tw2j).tolist()
            if (i, j) in ((0, 0), (1, 4)):                                      # the restatement of two of the ten
                want = RR.project(X, C, K, Rw2j, Tw2j, H, W)["image_u8"]
                assert np.array_equal(np.asarray(f["image"]), want), (i, j)
            assert np.array_equal(np.asarray(f["image"]), tensors["frames"][k]["image"].cpu().numpy()), (i, j)
            k += 1
    assert tensors["pcd_points"].is_cuda and torch.equal(tensors["pcd_points"], Xd)
    # e: a render pose that looks away from the cloud has no valid point in any inner pose and is skipped (:544)
    away = render.copy()
    away[1, :3, :3] = np.diag([-1.0, 1.0, -1.0]) @ render[1, :3, :3]
    away[1, :3, 3:] = np.diag([-1.0, 1.0, -1.0]) @ render[1, :3, 3:]
    for j in range(5):
        Rw2j, Tw2j = RR.compose_pose(inner[j, :3, :3], inner[j, :3, 3:4], away[1, :3, :3], away[1, :3, 3:4])
        assert not RR.project_points(X, K, Rw2j, Tw2j, H, W)[0].any()
    skipped = reproject.align_frames(Xd, Cd, K, away, inner, H, W, 0.9)
    assert len(skipped["frames"]) == 5
    assert [f["transform_matrix"] for f in skipped["frames"]] == [f["transform_matrix"] for f in data["frames"][:5]]
