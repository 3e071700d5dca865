"""GPU: the off-screen test in phase 1 of the pooled preprocess kernel (csrc/screen_cull.h, lr_tune_set("pcull", 0) = off).
It may only drop what the projection chain would drop, so with it on or off EVERY output keeps its bits: header words, radii,
instance counts, the binning's records of emitting rows, records and clamp bits of visible rows, ranges, emission order,
inst_gid and both images -- and the thread-per-Gaussian kernel, which has no such test, is the third party.  The scenes aim at
the test's own edge (splats just inside and just outside every side and corner of the tile grid), at pools in which it leaves
0 / 1 / 255 / 256 / 257 of the near-plane passers, a cloud that ends mid-pool, and at every variant of the kernel: raw mode,
anti-aliasing, the caller's own 3D covariances (test inert), quaternions of any norm, rows that are no numbers, a posed camera."""
import math

import numpy as np
import pytest
import torch

from luciddreamer_amd import _C, _lib, cameras, config, synthetic
from tests import helpers as hp
from tests.test_gpu_pool_pairs import _diag_quat, _shs, _unpack, _unproject
from tests.test_screen_cull_cpu import edge_cloud, posed_camera

pytestmark = pytest.mark.gpu

SIZES = [(256, 144), (250, 130)]


@pytest.fixture(autouse=True)
def _restore_knobs():
    yield
    _lib.tune_set("preprocess", -1)
    _lib.tune_set("pcull", -1)
    config.set_antialiasing(False)


def _forward(cloud, cam, dev, mode="plain", scale_modifier=1.0):
    tfx, tfy = hp.tan_fov(cam)
    c = cam.to(dev)
    e = torch.Tensor([])
    bg = torch.zeros(3, device=dev)
    d = lambda k: cloud[k].to(dev)
    H, W = cam.image_height, cam.image_width
    if mode == "raw":           # the stored tensors: log-scales, logit-opacities, quaternions as they are, SH split in two
        op = cloud["opacities"].clamp(1e-6, 1 - 1e-6)
        return _C.rasterize_gaussians_raw(bg, d("means3D"), cloud["shs"][:, :1, :].contiguous().to(dev),
                                          cloud["shs"][:, 1:, :].contiguous().to(dev), torch.log(op / (1 - op)).to(dev),
                                          torch.log(cloud["scales"]).to(dev), d("rotations"), scale_modifier, c.world_view_transform,
                                          c.full_proj_transform, tfx, tfy, H, W, 3, c.camera_center, False, binning_capacity=0)
    cov = mode == "cov"
    return _C.rasterize_gaussians(bg, d("means3D"), e, d("opacities"), e if cov else d("scales"), e if cov else d("rotations"),
                                  scale_modifier, d("cov3D") if cov else e, c.world_view_transform, c.full_proj_transform, tfx, tfy,
                                  H, W, d("shs"), 3, c.camera_center, False, False, binning_capacity=0)


def _same(a, b, what):
    assert a["num_rendered"] == b["num_rendered"], what
    for k in ("hdr", "radii", "tiles", "ranges", "emission", "inst_gid", "color", "depth"):
        assert np.array_equal(a[k], b[k]), (what, k)
    vis = a["radii"] != 0                                      # records and clamp bits exist for these only
    assert np.array_equal(a["rec"][vis], b["rec"][vis]) and np.array_equal(a["clamped"][vis], b["clamped"][vis]), what
    emit = a["tiles"] != 0                                     # the binning's record is read for the emitting ones only
    assert np.array_equal(a["hitrec"][emit], b["hitrec"][emit]), what


def _on_off(cloud, cam, dev, mode="plain", scale_modifier=1.0, third_party=True):
    """Pooled kernel with the test on and off, and the thread-per-Gaussian kernel: identical.  Returns the buffers."""
    P, W, H = cloud["means3D"].shape[0], cam.image_width, cam.image_height
    runs = {}
    for name, pre, cull in [("on", 1, -1), ("off", 1, 0)] + ([("plain", 0, -1)] if third_party else []):
        _lib.tune_set("preprocess", pre)
        _lib.tune_set("pcull", cull)
        runs[name] = _unpack(_forward(cloud, cam, dev, mode, scale_modifier), P, W, H)
    _lib.tune_set("preprocess", -1)
    _lib.tune_set("pcull", -1)
    _same(runs["off"], runs["on"], "test on against off")
    if third_party:
        _same(runs["plain"], runs["on"], "pooled with the test against one thread per Gaussian")
    return runs["on"]


def _cat(*clouds):
    return {k: torch.cat([c[k] for c in clouds]).contiguous() for k in clouds[0]}


def _filler(cam, P, rng, spread=3.0):
    """Random splats over `spread` screens around the view, a third of them behind the camera."""
    W, H = cam.image_width, cam.image_height
    focal = W / (2 * hp.tan_fov(cam)[0])
    z = rng.uniform(0.5, 6.0, P)
    z[rng.permutation(P)[:P // 3]] *= -1.0
    px, py = rng.uniform(-spread * W, (1 + spread) * W, P), rng.uniform(-spread * H, (1 + spread) * H, P)
    sig = np.exp(rng.uniform(math.log(0.3), math.log(40.0), (P, 3))) * np.abs(z)[:, None] / focal
    q = rng.standard_normal((P, 4))
    return dict(means3D=torch.from_numpy(_unproject(cam, px, py, z)), scales=torch.from_numpy(sig.astype(np.float32)),
                rotations=torch.from_numpy((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)),
                opacities=torch.from_numpy(rng.uniform(0.05, 1.0, (P, 1)).astype(np.float32)), shs=_shs(P, rng))


def _edge_scene(cam, rng, P):
    """The edge cloud of tests/test_screen_cull_cpu.py (with colours), shuffled among filler up to P rows."""
    edge, _, _, _ = edge_cloud(cam, rng)
    n = edge["means3D"].shape[0]
    edge["shs"] = _shs(n, rng)
    edge["opacities"] = torch.from_numpy(rng.uniform(0.05, 1.0, (n, 1)).astype(np.float32))
    cloud = _cat(edge, _filler(cam, P - n, rng))
    perm = torch.from_numpy(rng.permutation(P))
    return {k: v[perm].contiguous() for k, v in cloud.items()}


@pytest.mark.parametrize("size", SIZES)
def test_edge_cloud_on_off_and_thread_per_gaussian(hip_device, size):
    cam = cameras.identity_camera(*size)
    cloud = _edge_scene(cam, np.random.default_rng(21), 3 * 512 + 211)      # ends mid-pool
    u = _on_off(cloud, cam, hip_device)
    assert 100 < (u["radii"] > 0).sum() < 1200


def _fill_scene(cam, kept, tail, rng):
    """Pools of 512 near-plane passers of which the off-screen test leaves `kept`: those on the screen (thin diagonal splats,
    2 to 60 pixels) or within a radius of its edge; the others 40 screens away, where a bound of three radii cannot reach.
    Then a partial pool of `tail` rows, half of them behind the camera."""
    W, H = cam.image_width, cam.image_height
    sizes = list(kept) + [tail // 2]
    pools = [512] * len(kept) + [tail]
    P = sum(pools)
    alive = np.zeros(P, bool)
    o = 0
    for c, n in zip(sizes, pools):
        alive[o + rng.permutation(n)[:c]] = True
        o += n
    z = rng.uniform(2.0, 6.0, P)
    px, py = rng.uniform(-6, W + 6, P), rng.uniform(-6, H + 6, P)
    dead = np.nonzero(~alive)[0]
    side = rng.integers(0, 4, dead.size)
    px[dead] = np.where(side == 0, -40.0 * W, np.where(side == 1, 41.0 * W, px[dead]))
    py[dead] = np.where(side == 2, -40.0 * H, np.where(side == 3, 41.0 * H, py[dead]))
    z[512 * len(kept) + np.nonzero(~alive[512 * len(kept):])[0][::2]] = -1.0       # the tail's: also some behind the near plane
    focal = W / (2 * hp.tan_fov(cam)[0])
    major = rng.uniform(0.4, 20.0, P) * np.abs(z) / focal
    scales = np.stack([major, 0.02 * major, 0.02 * major], axis=1).astype(np.float32)
    opac = rng.uniform(0.02, 1.0, (P, 1)).astype(np.float32)
    return dict(means3D=torch.from_numpy(_unproject(cam, px, py, z)), scales=torch.from_numpy(scales), rotations=_diag_quat(P),
                opacities=torch.from_numpy(opac), shs=_shs(P, rng)), alive


@pytest.mark.parametrize("size", SIZES)
def test_pools_of_every_fill_after_the_test(hip_device, size):
    cam = cameras.identity_camera(*size)
    kept = [0, 1, 255, 256, 257]
    cloud, alive = _fill_scene(cam, kept, 300, np.random.default_rng(22))       # 5 * 512 + 300 rows
    u = _on_off(cloud, cam, hip_device)
    assert not (u["radii"][~alive] != 0).any()                 # what was put 40 screens away is gone either way
    got = [int((u["radii"][512 * k:512 * (k + 1)] > 0).sum()) for k in range(len(kept))]
    assert all(g <= k for g, k in zip(got, kept)) and sum(got) > 0.8 * sum(kept), got      # (a few of the kept lie just outside the edge)


def _band_scene(P, size, seed, view=1):
    cloud = synthetic.make_cloud(P, "band", seed, scale_mult=0.5)
    return cloud, cameras.rotate360_path(size[0], size[1], n_views=6)[view]


@pytest.mark.parametrize("size", SIZES)
def test_raw_mode(hip_device, size):
    cloud, cam = _band_scene(4096, size, 3)
    g = torch.Generator().manual_seed(5)
    cloud["rotations"] = cloud["rotations"] * (0.5 + 1.5 * torch.rand(4096, 1, generator=g))       # normalised by the kernel
    u = _on_off(cloud, cam, hip_device, mode="raw")
    assert (u["radii"] > 0).sum() > 100


@pytest.mark.parametrize("size", SIZES)
def test_antialiasing(hip_device, size):
    cam = cameras.identity_camera(*size)
    cloud = _edge_scene(cam, np.random.default_rng(23), 2048 + 100)
    config.set_antialiasing(True)
    u = _on_off(cloud, cam, hip_device)
    config.set_antialiasing(False)
    assert (u["radii"] > 0).sum() > 100


def test_own_covariances_leave_the_test_inert(hip_device):
    """cov3D_precomp need not be positive semi-definite (tests/test_gpu_pool_pairs.py feeds indefinite ones): no bound holds
    for them, so the kernel does not test -- scales and rotations are not even given."""
    W, H = SIZES[1]
    cam = cameras.identity_camera(W, H)
    rng = np.random.default_rng(24)
    P = 2000
    focal = W / (2 * hp.tan_fov(cam)[0])
    z = rng.uniform(2.0, 6.0, P)
    var = (rng.uniform(0.5, 8.0, (P, 3)) * (z / focal)[:, None]) ** 2
    var[rng.permutation(P)[:P // 3], 0] *= -1.0
    cov = np.zeros((P, 6), np.float32)
    cov[:, 0], cov[:, 3], cov[:, 5] = var[:, 0], var[:, 1], var[:, 2]
    cov[:, 1] = 0.3 * np.sqrt(np.abs(var[:, 0] * var[:, 1])) * rng.uniform(-1, 1, P)
    cloud = dict(means3D=torch.from_numpy(_unproject(cam, rng.uniform(-2 * W, 3 * W, P), rng.uniform(-2 * H, 3 * H, P), z)),
                 cov3D=torch.from_numpy(cov), opacities=torch.from_numpy(rng.uniform(0.02, 1.0, (P, 1)).astype(np.float32)),
                 shs=_shs(P, rng))
    u = _on_off(cloud, cam, hip_device, mode="cov")
    assert (u["radii"] > 0).sum() > 100


@pytest.mark.parametrize("norm", [0.5, 2.0])
def test_quaternions_of_any_norm(hip_device, norm):
    cam = cameras.identity_camera(*SIZES[1])
    cloud = _edge_scene(cam, np.random.default_rng(25), 1536)
    cloud["rotations"] = cloud["rotations"] * norm
    for mod in (1.0, 3.0):
        u = _on_off(cloud, cam, hip_device, scale_modifier=mod)
        assert (u["radii"] > 0).sum() > 100


def test_rows_that_are_no_numbers(hip_device):
    """NaN / inf / 0 / negative scales, NaN means, NaN quaternions among ordinary rows: the test lets them through, and what
    the chain makes of them it makes with the test on or off."""
    cam = cameras.identity_camera(*SIZES[0])
    rng = np.random.default_rng(26)
    P = 1536 + 64
    cloud = _filler(cam, P, rng, spread=1.5)
    rows = torch.from_numpy(rng.permutation(P)[:80])
    g = [rows[i::8] for i in range(8)]
    nan, inf = float("nan"), float("inf")
    cloud["scales"][g[0], 0] = nan; cloud["scales"][g[1], 2] = nan
    cloud["scales"][g[2], 1] = inf
    cloud["scales"][g[3]] = 0.0
    cloud["scales"][g[4]] *= -1.0
    cloud["means3D"][g[5], 0] = nan; cloud["means3D"][g[6], 2] = nan
    cloud["rotations"][g[7], 1] = nan
    u = _on_off(cloud, cam, hip_device)
    assert (u["radii"] > 0).sum() > 100


@pytest.mark.parametrize("size", SIZES)
def test_posed_camera(hip_device, size):
    cam = posed_camera(*size)
    ident = cameras.identity_camera(*size)
    cloud = _edge_scene(ident, np.random.default_rng(27), 3000)
    c2w = torch.inverse(cam.world_view_transform.T.double())
    cloud["means3D"] = (cloud["means3D"].double() @ c2w[:3, :3].T + c2w[:3, 3]).float().contiguous()
    u = _on_off(cloud, cam, hip_device)
    assert (u["radii"] > 0).sum() > 100


def test_one_multi_view_call(hip_device):
    """ViewBatch, 4 views of the rotate path, P = 4096, 128 x 128: the gradient bucket and the means2D accumulator of the step
    have the same bits with the test on and off."""
    from luciddreamer_amd import parallel
    P, W, H = 4096, 128, 128
    cloud = synthetic.make_cloud(P, "band", 8, scale_mult=0.5)
    cams = [c.to(hip_device) for c in cameras.rotate360_path(W, H, n_views=4)]
    g = synthetic.upstream_grad(H, W).to(hip_device)
    bg = torch.tensor([0.1, 0.0, 0.2], device=hip_device)
    det = {k: v.to(hip_device) for k, v in cloud.items()}
    shapes = {"means3D": (P, 3), "means2D": (P, 3), "opacity": (P, 1), "sh": (P, 16, 3), "scales": (P, 3), "rotations": (P, 4)}
    results = {}
    _lib.tune_set("preprocess", 1)
    _lib.tune_set("blend_quad", 2)       # the blend shapes pinned, as wherever steps are compared to the bit
    _lib.tune_set("fwd_pair", 2)
    try:
        for cull in (-1, 0):
            _lib.tune_set("pcull", cull)
            batch = parallel.ViewBatch(cams, [g] * len(cams), 3, bg, binning_capacity=100_000, n_streams=2)
            acc = {k: torch.zeros(s, device=hip_device) for k, s in shapes.items()}
            with torch.no_grad():
                batch.run(det["means3D"], det["opacities"], det["scales"], det["rotations"], det["shs"], acc)
            batch.check()
            results[cull] = {k: v.cpu() for k, v in acc.items()}
    finally:
        _lib.tune_set("blend_quad", -1)
        _lib.tune_set("fwd_pair", -1)
    for k in shapes:
        assert torch.equal(results[-1][k], results[0][k]), k
    assert float(results[-1]["means2D"].abs().max()) > 0 and float(results[-1]["scales"].abs().max()) > 0
