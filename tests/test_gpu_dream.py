"""Dreaming on the GPU (csrc/dream.hip through luciddreamer_amd.reproject) against the numpy restatement (tests/dream_ref.py) on
the same inputs.  Everything but the scale sums' bound is compared for exact equality: float64 expressions in one documented
order.  The shapes are the smallest at which each kernel can still go wrong: more than one workgroup, sizes that are no multiple
of the workgroup or of the sample tile, every sample count around a tile's edge, waves whose lanes diverge."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import dream_ref as DR
from tests import reproject_ref as RR

pytestmark = pytest.mark.gpu

TILE = DR.BLOCK


def _pose(rng, shift=0.1):
    a, b, c = rng.uniform(-0.08, 0.08, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rx @ Ry @ Rz, rng.uniform(-shift, shift, (3, 1))


def _intrinsics(H, W):
    return np.array([[0.9 * W, 0, W / 2.0], [0, 0.9 * W, H / 2.0], [0, 0, 1]], dtype=np.float64)


def _depth_map(seed, H, W):
    """What a depth network would hand over: smooth, near the cloud's layers, float32."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    return (3.4 + 0.5 * np.sin(x / W * 3.0) + 0.4 * np.cos(y / H * 2.0) + rng.uniform(0, 0.01, (H, W))).astype(np.float32)


_SCENES = {}


def _scene(H, W, N):
    """A cloud in two depth layers over two thirds of the view (holes and a border on the rest), its restated frame, a depth
    map and an image; computed once and shared, never changed."""
    key = (H, W, N)
    if key not in _SCENES:
        rng = np.random.default_rng(H * 1000 + N)
        K = _intrinsics(H, W)
        R, T = _pose(rng)
        u = np.concatenate([rng.uniform(-6, 0.68 * W, N - 25), rng.uniform(0.68 * W, W + 4, 25)])
        v = rng.uniform(-6, H + 5, N)
        z = np.where(rng.random(N) < 0.5, rng.uniform(2.8, 3.2, N), rng.uniform(5.5, 6.5, N))
        z[rng.random(N) < 0.02] *= -1
        cam = np.linalg.inv(K) @ np.stack([u * z, v * z, z])
        X = np.ascontiguousarray((np.linalg.inv(R) @ (cam - T)).astype(np.float32))
        C = rng.random((N, 3)).astype(np.float32)
        fr = RR.project(X, C, K, R, T, H, W)
        assert 0 < fr["mask"].sum() < H * W and fr["border"].any() and 0 < fr["valid"].sum() < N
        _SCENES[key] = dict(H=H, W=W, N=N, X=X, C=C, K=K, R=R, T=T, fr=fr, D=_depth_map(N, H, W),
                            image=rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
    return _SCENES[key]


def _frame(dev, s, X=None):
    from luciddreamer_amd import reproject
    X = s["X"] if X is None else X
    f = reproject.project(torch.from_numpy(X).to(dev), torch.from_numpy(s["C"]).to(dev), s["K"], s["R"], s["T"], s["H"], s["W"])
    assert np.array_equal(f.valid.cpu().numpy(), s["fr"]["valid"]) and np.array_equal(f.pix.cpu().numpy(), s["fr"]["pix"])
    return f


def _same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


# ---- 1: scale sums ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [0, 1])                                       # N = 3 H W, and one fewer: no multiple of 256
def test_1_scale_sums(hip_device, drop):
    """|S - fsum| <= n 2^-53 sum |term|: the bound of a float64 sum of n terms in any order, both sides from the restatement's
    terms.  The count is exact, and the sums equal the restatement's in the documented order to the bit."""
    from luciddreamer_amd import reproject
    H, W = 48, 64
    s = _scene(H, W, 3 * H * W - drop)
    f = _frame(hip_device, s)
    Xd = torch.from_numpy(s["X"]).to(hip_device)
    for bad in (False, True):
        D = s["D"].copy()
        lost = 0
        if bad:                                                                # a NaN and an inf under valid points
            pix = s["fr"]["pix"][np.nonzero(s["fr"]["valid"])[0][[5, 1500]]]
            D.reshape(-1)[pix[0]], D.reshape(-1)[pix[1]] = np.nan, np.inf
            lost = int((np.isin(s["fr"]["pix"], pix) & (s["fr"]["valid"] != 0)).sum())
            assert lost >= 2
        fit = reproject.fit_scale(Xd, f, torch.from_numpy(D).to(hip_device), s["K"], s["R"], s["T"])
        pp, pq, qq, use = DR.scale_terms(s["X"], s["fr"]["valid"], s["fr"]["pix"], D, s["K"], s["R"], s["T"], H, W)
        n = int(use.sum())
        assert fit.n_used == n == int(s["fr"]["valid"].sum()) - lost
        for got, term, name in ((fit.spp, pp, "spp"), (fit.spq, pq, "spq"), (fit.sqq, qq, "sqq")):
            bound = n * 2.0 ** -53 * math.fsum(np.abs(term))
            print(name, "device", got, "fsum", math.fsum(term), "bound", bound)
            assert np.isfinite(got) and abs(got - math.fsum(term)) <= bound, name
        want = DR.scale_sums(s["X"], s["fr"]["valid"], s["fr"]["pix"], D, s["K"], s["R"], s["T"], H, W)
        assert (fit.spp, fit.spq, fit.sqq, fit.n_used) == want
        scale, before, after = DR.fit_from_sums(*want)
        assert (fit.scale, fit.mse_before, fit.mse_after) == (scale, before, after) and after <= before
        again = reproject.fit_scale(Xd, f, torch.from_numpy(D).to(hip_device), s["K"], s["R"], s["T"])
        assert again == fit                                                    # two runs: equal bits
    # [N,3] input: the same sums
    rows = reproject.fit_scale(torch.from_numpy(np.ascontiguousarray(s["X"].T)).to(hip_device), f,
                               torch.from_numpy(s["D"]).to(hip_device), s["K"], s["R"], s["T"])
    assert (rows.spp, rows.spq, rows.sqq, rows.n_used) == DR.scale_sums(s["X"], s["fr"]["valid"], s["fr"]["pix"], s["D"], s["K"],
                                                                        s["R"], s["T"], H, W)


def test_1_scale_sums_of_an_empty_cloud(hip_device):
    from luciddreamer_amd import reproject
    H, W = 20, 30
    K, R, T = _intrinsics(H, W), np.eye(3), np.zeros((3, 1))
    X = torch.zeros((3, 0), device=hip_device)
    f = reproject.project(X, torch.zeros((0, 3), device=hip_device), K, R, T, H, W)
    fit = reproject.fit_scale(X, f, torch.ones((H, W), device=hip_device), K, R, T)
    assert fit == reproject.ScaleFit(1.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)


# ---- 2: correspondences ----------------------------------------------------------------------------------------------------------
def _correspond_device(dev, s, pix, corr, D, scale):
    from luciddreamer_amd import _lib, reproject
    X = torch.from_numpy(s["X"]).to(dev)
    pixd, Dd = torch.from_numpy(pix).to(dev), torch.from_numpy(D).to(dev)
    corrd = torch.from_numpy(corr).to(dev)
    M = int(corr.shape[0])
    out = torch.full((3, M + 4), -7.0, dtype=torch.float64, device=dev)
    pose = reproject._Pose(s["K"], s["R"], s["T"])
    args = _lib.DreamArgs(n_points=s["N"], points=X.data_ptr(), point_stride=1, coord_stride=s["N"], pix=pixd.data_ptr(),
                          height=s["H"], width=s["W"], depth=Dd.data_ptr(), scale=scale, corr=corrd.data_ptr() if M else None,
                          n_corr=M, out_su=out[0].data_ptr(), out_sv=out[1].data_ptr(), out_sval=out[2].data_ptr(),
                          stream=torch.cuda.current_stream(dev).cuda_stream, **pose.fields())
    assert _lib.lib().lr_dream_correspond(ctypes.byref(args)) == 0, _lib.last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("M, scale", [(0, 1.0), (1, 1.0), (TILE + 1, 1.0), (TILE + 1, 1.0625), (2 * TILE + 3, 0.93)])
def test_2_correspondences(hip_device, M, scale):
    H, W = 48, 64
    s = _scene(H, W, 3 * H * W)
    valid_idx = np.nonzero(s["fr"]["valid"])[0]
    corr = valid_idx[np.linspace(0, valid_idx.shape[0] - 1, M).astype(np.int64)].astype(np.int32) if M else np.zeros(0, np.int32)
    assert np.unique(corr).shape[0] == M
    D = s["D"].copy()
    if M > 1:
        D.reshape(-1)[s["fr"]["pix"][corr[M // 2]]] = 0.0                     # a depth-0 pixel under a correspondence
    got = _correspond_device(hip_device, s, s["fr"]["pix"], corr, D, scale)
    su, sv, sval = DR.correspond(s["X"], s["fr"]["pix"], corr, D, s["K"], s["R"], s["T"], H, W, scale)
    assert _same_bits(got[0], su) and _same_bits(got[1], sv) and _same_bits(got[2], sval)
    assert np.array_equal(got[:, M:], [[0, 0, W - 1, W - 1], [0, H - 1, 0, H - 1], [0, 0, 0, 0]])      # the corners, last, in order
    if M > 1 and scale == 1.0:
        zero = np.nonzero(s["fr"]["pix"][corr] == s["fr"]["pix"][corr[M // 2]])[0]
        assert np.isnan(got[2][zero]).all() and np.isfinite(got[2][np.setdiff1d(np.arange(M), zero)]).all()
    if M:
        assert np.isfinite(got[:2]).all() and np.abs(np.rint(got[0][:M]) + W * np.rint(got[1][:M]) - s["fr"]["pix"][corr]).max() == 0


# ---- 3: interpolation ------------------------------------------------------------------------------------------------------------
def _where(kind, H, W):
    if kind == "all":
        return np.zeros((H, W), dtype=np.uint8)
    if kind == "none":
        return np.full((H, W), 3, dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    return (((x + y) % 2) * 255).astype(np.uint8)                              # checkerboard: the lanes of a wave diverge


def _scatter_both(dev, su, sv, sval, H, W, where):
    from luciddreamer_amd import reproject
    uv = torch.from_numpy(np.ascontiguousarray(np.stack([su, sv], axis=1).reshape(-1, 2))).to(dev)
    got = reproject.scatter_interpolate(uv, torch.from_numpy(np.ascontiguousarray(sval)).to(dev), H, W, torch.from_numpy(where).to(dev))
    want = DR.scatter(su, sv, sval, H, W, where)
    assert got.dtype == torch.float32 and tuple(got.shape) == (H, W)
    g = got.cpu().numpy()
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), int((g.view(np.uint32) != want.view(np.uint32)).sum())
    assert (g[where != 0] == 0).all()
    return g


def _random_samples(M, H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, W, M), rng.uniform(-1.0, H, M), rng.uniform(-0.5, 1.5, M)


@pytest.mark.parametrize("kind", ["all", "none", "checker"])
@pytest.mark.parametrize("M", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@pytest.mark.parametrize("H, W", [(48, 64), (37, 53)])
def test_3_interpolation_equals_the_restatement(hip_device, H, W, M, kind):
    su, sv, sval = _random_samples(M, H, W, 100 * M + H)
    where = _where(kind, H, W)
    g = _scatter_both(hip_device, su, sv, sval, H, W, where)
    if M == 0 or kind == "none":
        assert not g.any()
    else:
        q = g[where == 0]
        assert q.any() and q.min() >= np.float32(sval.min()) and q.max() <= np.float32(sval.max())


@pytest.mark.parametrize("kind", ["all", "checker"])
def test_3_corner_samples_alone_give_exactly_zero(hip_device, kind):
    H, W = 48, 64
    su, sv, sval = np.array([0.0, 0, W - 1, W - 1]), np.array([0.0, H - 1, 0, H - 1]), np.zeros(4)
    g = _scatter_both(hip_device, su, sv, sval, H, W, _where(kind, H, W))
    assert (g.view(np.uint32) == 0).all()


@pytest.mark.parametrize("H, W", [(48, 64), (37, 53)])
def test_3_special_samples(hip_device, H, W):
    ALL = _where("all", H, W)
    # a query exactly on a sample
    su, sv, sval = _random_samples(TILE + 9, H, W, 7)
    su[3], sv[3], su[TILE + 2], sv[TILE + 2] = 10.0, 5.0, 30.0, 20.0
    g = _scatter_both(hip_device, su, sv, sval, H, W, ALL)
    assert g[5, 10] == np.float32(sval[3]) and g[20, 30] == np.float32(sval[TILE + 2])
    # collinear samples: Shepard's mean everywhere
    t = np.linspace(2.0, W - 3.0, 40)
    su, sv, sval = t, 4.0 + 0.5 * t, np.sin(t / 7.0)
    assert DR.scatter_takes_fallback(su, sv, sval, H, W, ALL).all()
    _scatter_both(hip_device, su, sv, sval, H, W, _where("checker", H, W))
    # a NaN sample in the middle of a tile (and one at a tile's first and last place)
    su, sv, sval = _random_samples(2 * TILE + 50, H, W, 9)
    sval[[TILE // 2, TILE, 2 * TILE - 1, 2 * TILE + 20]] = np.nan
    g = _scatter_both(hip_device, su, sv, sval, H, W, _where("checker", H, W))
    keep = ~np.isnan(sval)
    assert np.array_equal(g, DR.scatter(su[keep], sv[keep], sval[keep], H, W, _where("checker", H, W)))
    # nothing but NaN: no sample is usable
    assert not _scatter_both(hip_device, su[:TILE + 1], sv[:TILE + 1], np.full(TILE + 1, np.nan), H, W, ALL).any()


# ---- 4: compensated lift ---------------------------------------------------------------------------------------------------------
def _lift_device(dev, D, nd, K, R, T, scale):
    from luciddreamer_amd import _lib, reproject
    H, W = D.shape
    Dd, ndd = torch.from_numpy(D).to(dev), torch.from_numpy(nd).to(dev)
    out = torch.empty((3, H * W), dtype=torch.float32, device=dev)
    pose = reproject._Pose(K, R, T)
    args = _lib.DreamArgs(height=H, width=W, depth=Dd.data_ptr(), new_depth=ndd.data_ptr(), out_points=out.data_ptr(), scale=scale,
                          stream=torch.cuda.current_stream(dev).cuda_stream, **pose.fields())
    assert _lib.lib().lr_dream_lift(ctypes.byref(args)) == 0, _lib.last_error()
    return out


@pytest.mark.parametrize("H, W", [(48, 64), (37, 53)])
def test_4_compensated_lift(hip_device, H, W):
    from luciddreamer_amd import reproject
    rng = np.random.default_rng(H)
    K = _intrinsics(H, W)
    R, T = _pose(rng)
    D = _depth_map(H, H, W)
    D[3, 5], D[10, 10] = 0.0, -1.0
    nd = (rng.uniform(-0.3, 0.3, (H, W)) * (rng.random((H, W)) < 0.5)).astype(np.float32)
    for scale in (1.0, 1.0625, 0.9371):
        got = _lift_device(hip_device, D, nd, K, R, T, scale).cpu().numpy()
        want = DR.dream_lift(D, nd, K, R, T, scale)
        assert got.shape == (3, H * W) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), scale
    plain = _lift_device(hip_device, D, np.zeros((H, W), dtype=np.float32), K, R, T, 1.0)
    assert torch.equal(plain, reproject.lift(torch.from_numpy(D).to(hip_device), K, R, T))


# ---- 5, 6: dream_step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["lstsq", "reference", 1.0625])
def test_5_dream_step_equals_the_restatement(hip_device, scale, monkeypatch):
    from luciddreamer_amd import reproject
    H, W = 48, 64
    s = _scene(H, W, 3 * H * W)
    N = s["N"]
    f = _frame(hip_device, s)
    dev = hip_device
    want_p, want_c, info = DR.dream_step(s["X"], s["C"], s["fr"], s["image"], s["D"], s["K"], s["R"], s["T"], H, W, scale)
    n_hole = int((s["fr"]["mask"] == 0).sum())
    assert info["n_added"] == n_hole > 0 and info["n_corr"] > 0
    if scale == "reference":                                                   # no fit is launched
        monkeypatch.setattr(reproject, "fit_scale", lambda *a, **k: pytest.fail("scale='reference' ran the fit"))
    Cd, Dd = torch.from_numpy(s["C"]).to(dev), torch.from_numpy(s["D"]).to(dev)
    for X, image in ((s["X"], s["image"]), (np.ascontiguousarray(s["X"].T), s["image"]),
                     (s["X"], s["image"].astype(np.float32) / 255.)):
        pts, cols, got = reproject.dream_step(torch.from_numpy(X).to(dev), Cd, f, torch.from_numpy(image).to(dev), Dd, s["K"],
                                              s["R"], s["T"], scale=scale)
        assert tuple(pts.shape) == (3, N + n_hole) and tuple(cols.shape) == (N + n_hole, 3)
        assert got.n_added == n_hole == int((f.mask == 0).sum()) and got.n_corr == info["n_corr"] and got.scale == info["scale"]
        assert _same_bits(pts, want_p) and _same_bits(cols, want_c)
        if scale == "lstsq":
            assert (got.fit.spp, got.fit.spq, got.fit.sqq, got.fit.n_used) == info["sums"] and got.fit.scale == got.scale
        else:
            assert got.fit is None and got.scale == (1.0 if scale == "reference" else scale)
    # row-major order: the appended points are the compensated lift at the hole pixels, in np.where order
    comp = reproject.compensate(torch.from_numpy(s["X"]).to(dev), f, Dd, s["K"], s["R"], s["T"], scale=info["scale"])
    hole = np.nonzero(s["fr"]["mask"].reshape(-1) == 0)[0]
    assert np.array_equal(pts.cpu().numpy()[:, N:], comp.lifted.cpu().numpy()[:, hole])
    assert _same_bits(comp.new_depth, info["comp"]["new_depth"]) and _same_bits(comp.lifted, info["comp"]["lifted"])
    assert _same_bits(comp.corr_uv, np.stack([info["comp"]["su"], info["comp"]["sv"]], axis=1))
    assert _same_bits(comp.corr_value, info["comp"]["sval"]) and comp.n_corr == info["n_corr"]
    assert (comp.new_depth.cpu().numpy()[s["fr"]["mask"] == 1] == 0).all() and comp.new_depth.cpu().numpy().any()


def test_5_a_depth_map_off_by_a_scale_is_brought_back(hip_device):
    """The cloud is the lift of a depth map D0 at a pose with T = 0 (the scale acts about the world's origin, as the reference's
    trans3d does) with a block of points removed; the network's depth is D0 / 1.1.  Every pair has q = P / 1.1 up to two float32
    roundings (of the point and of D0 / 1.1: 1.2e-7 relative), so the fitted scale is within 1.1 x 1.2e-7 < 1e-6 of 1.1; the
    offsets along the border are then float32 rounding noise, and the compensation inside the mask is 0."""
    from luciddreamer_amd import reproject
    H, W = 48, 64
    rng = np.random.default_rng(77)
    K = _intrinsics(H, W)
    R, _ = _pose(rng)
    T = np.zeros((3, 1))
    D0 = _depth_map(5, H, W)
    keep = np.ones((H, W), dtype=bool)
    keep[12:32, 20:44] = False
    X = np.ascontiguousarray(RR.lift(D0, K, R, T)[:, keep.reshape(-1)])
    C = rng.random((X.shape[1], 3)).astype(np.float32)
    dev = hip_device
    Xd, Cd = torch.from_numpy(X).to(dev), torch.from_numpy(C).to(dev)
    f = reproject.project(Xd, Cd, K, R, T, H, W)
    n_hole = int((f.mask == 0).sum())
    assert 0 < n_hole < 20 * 24 + 200
    D = (D0 / np.float32(1.1)).astype(np.float32)
    image = torch.from_numpy(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).to(dev)
    pts, cols, info = reproject.dream_step(Xd, Cd, f, image, torch.from_numpy(D).to(dev), K, R, T)
    assert abs(info.scale - 1.1) <= 1e-6 and info.fit.mse_after <= info.fit.mse_before and info.fit.n_used == int(f.valid.sum())
    assert info.n_added == n_hole and info.n_corr > 0 and tuple(pts.shape) == (3, X.shape[1] + n_hole)
    comp = reproject.compensate(Xd, f, torch.from_numpy(D).to(dev), K, R, T, scale=info.scale)
    assert (comp.new_depth[f.mask == 1] == 0).all()
    print("largest border offset", float(comp.corr_value.abs().max()))
    assert float(comp.corr_value.abs().max()) <= 1e-4                          # 7 units of depth x a few float32 roundings
    hole = (f.mask.reshape(-1) == 0).nonzero()[:, 0]
    truth = torch.from_numpy(RR.lift(D0, K, R, T)).to(dev)[:, hole]
    assert float((pts[:, X.shape[1]:] - truth).abs().max()) <= 1e-3            # the removed block is put back where it was


def test_6_two_runs_give_the_same_bits(hip_device):
    from luciddreamer_amd import reproject
    H, W = 48, 64
    s = _scene(H, W, 3 * H * W)
    f = _frame(hip_device, s)
    args = [torch.from_numpy(s[k]).to(hip_device) for k in ("X", "C")] + [f] + \
           [torch.from_numpy(s[k]).to(hip_device) for k in ("image", "D")] + [s["K"], s["R"], s["T"]]
    a, b = reproject.dream_step(*args), reproject.dream_step(*args)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert a[2] == b[2]


# ---- 7: errors -------------------------------------------------------------------------------------------------------------------
def test_7_errors_come_before_any_launch(hip_device):
    from luciddreamer_amd import _lib, reproject
    H, W = 37, 53
    s = _scene(H, W, 3 * H * W)
    dev = hip_device
    f = _frame(dev, s)
    X, C, D, img = (torch.from_numpy(s[k]).to(dev) for k in ("X", "C", "D", "image"))
    K, R, T = s["K"], s["R"], s["T"]
    batch = reproject.project_batch(X, C, K, np.stack([R, R]), np.stack([T, T]), H, W)
    for call in (lambda **k: reproject.fit_scale(k.get("X", X), k.get("f", f), k.get("D", D), K, R, T),
                 lambda **k: reproject.compensate(k.get("X", X), k.get("f", f), k.get("D", D), K, R, T),
                 lambda **k: reproject.dream_step(k.get("X", X), C, k.get("f", f), img, k.get("D", D), K, R, T)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call(D=D.cpu())
        with pytest.raises(RuntimeError, match="HIP device"):
            call(X=X.cpu())
        with pytest.raises(ValueError, match="one pose"):
            call(f=batch)
        with pytest.raises(ValueError, match="depth must be float32"):
            call(D=D[:, :-1].contiguous())
        with pytest.raises(ValueError, match="depth must be float32"):
            call(D=D.double())
        with pytest.raises(ValueError, match="projected from"):
            call(X=X[:, :-1].contiguous())
    with pytest.raises(ValueError, match="scale must be"):
        reproject.dream_step(X, C, f, img, D, K, R, T, scale="adam")
    with pytest.raises(ValueError, match="image must be"):
        reproject.dream_step(X, C, f, img[:, :-1].contiguous(), D, K, R, T)
    with pytest.raises(ValueError, match="uv must be float64"):
        reproject.scatter_interpolate(torch.zeros((3, 2), device=dev), torch.zeros(3, dtype=torch.float64, device=dev), H, W, f.mask)
    with pytest.raises(ValueError, match="where must be"):
        reproject.scatter_interpolate(torch.zeros((3, 2), dtype=torch.float64, device=dev),
                                      torch.zeros(3, dtype=torch.float64, device=dev), H, W + 1, f.mask)
    # a wrong struct_bytes: LR_ERR_INVALID_ARG, and the outputs are untouched
    L = _lib.lib()
    out = torch.full((H, W), 5.0, device=dev)
    uv = torch.zeros((2, 4), dtype=torch.float64, device=dev)
    sa = _lib.ScatterArgs(n_samples=4, su=uv[0].data_ptr(), sv=uv[1].data_ptr(), sval=uv[0].data_ptr(), height=H, width=W,
                          where=f.mask.data_ptr(), out=out.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    sa.struct_bytes -= 8
    assert L.lr_scatter_interpolate(ctypes.byref(sa)) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    lifted = torch.full((3, H * W), 5.0, device=dev)
    pose = reproject._Pose(K, R, T)
    da = _lib.DreamArgs(height=H, width=W, depth=D.data_ptr(), new_depth=D.data_ptr(), out_points=lifted.data_ptr(), scale=1.0,
                        stream=torch.cuda.current_stream(dev).cuda_stream, **pose.fields())
    da.struct_bytes += 8
    for fn in (L.lr_dream_lift, L.lr_dream_correspond, L.lr_dream_scale_sums):
        assert fn(ctypes.byref(da)) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    torch.cuda.synchronize()
    assert (out == 5.0).all() and (lifted == 5.0).all()
