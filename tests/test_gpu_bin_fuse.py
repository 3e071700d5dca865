"""GPU: the per-bin sort in ONE launch (tilebin.hip k_tile_sort_resid; async mode, lr_tune_set("bin_fuse", -1 / 1)) against the
two launches it replaces ("bin_fuse" 0: k_tile_sort_small + k_tile_sort_large, which the parity tests hold to the oracle), inside
one build and BYTE FOR BYTE.  Where the average bin is small -- a capacity of at most 256 entries per tile asks for that here --
the part-B workgroups of the small sort's grid also serve the queue of the bins of more than 1024 entries and sort them in place;
with a larger capacity the launch rule keeps the two launches, and both knob values must run the same kernels.

Compared: the header words, the forward-log words, vis_list, offsets, ranges, point_list, list_gid, inst_gid, radii and the
images; for the multi-view step every accumulator.  Scenes: one tile of EXACTLY n entries around every size class of the per-bin
sort and of the in-place sort (one, two and three blocks of 1024, the last one partial), distinct depths and groups of equal
ones; three queued bins beside small ones; a view that overflows its capacity; a step of four views on three chains, run twice;
an image of more than 16384 tiles (a bin is two tiles: the sort writes the ranges); both shapes of the blend forward."""
import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, cameras
from tests import helpers as hp
from tests.test_gpu_step_invariants import ACC_SHAPES, _assert_same, _host_array, _scene as _step_scene

pytestmark = pytest.mark.gpu

W, H = 64, 48                                   # 4 x 3 tiles
KNOBS = [0, 1, -1]                                 # the five launches first: the reference of every comparison


@pytest.fixture(autouse=True)
def _restore_knobs():
    yield
    _lib.tune_set("bin_fuse", -1)
    _lib.tune_set("fwd_pair", -1)


def _align(n):
    return (n + 255) // 256 * 256


def _forward(cloud, cam, dev, capacity):
    from luciddreamer_amd import _C
    tfx, tfy = hp.tan_fov(cam)
    c = cam.to(dev)
    e = torch.Tensor([])
    out = _C.rasterize_gaussians(torch.tensor([0.1, 0.0, 0.2], device=dev), cloud["means3D"].to(dev), e, cloud["opacities"].to(dev),
                                 cloud["scales"].to(dev), cloud["rotations"].to(dev), 1.0, e, c.world_view_transform,
                                 c.full_proj_transform, tfx, tfy, cam.image_height, cam.image_width,
                                 cloud["shs"].to(dev), 3, c.camera_center, False, False, binning_capacity=capacity)
    log = _C.header_poll(_C.last_forward_ticket(), True)
    return out, list(log)


def _unpack(out, log, P, w, h):
    """csrc/common.h geom / img / bin layouts, as tests/test_gpu_pool_pairs.py and tests/test_gpu_rank_sort.py read them."""
    _, color, depth, radii, geom, binning, img = out
    g = geom.cpu().numpy()
    hdr = g[:256].view(np.uint32).copy()
    n_compact, n_sorted, Rb = int(hdr[8]), int(hdr[5]), max(int(hdr[7]), 1)
    o = 256
    rec = g[o:o + 48 * P].view(np.uint32).reshape(P, 12).copy(); o += _align(48 * P)
    o += _align(P)
    tiles = g[o:o + 4 * P].view(np.uint32).copy(); o += _align(4 * P)
    vis_list = g[o:o + 4 * n_compact].view(np.uint32).copy(); o += _align(4 * P)
    offsets = g[o:o + 4 * n_compact].view(np.uint32).copy()
    N, T = w * h, ((w + 15) // 16) * ((h + 15) // 16)
    im = img.cpu().numpy()
    ranges = im[2 * _align(4 * N):2 * _align(4 * N) + 8 * T].view(np.uint32).reshape(T, 2).copy()
    b = binning.cpu().numpy()
    emission = b[:4 * n_sorted].view(np.uint32).copy()
    gid_off = _align(4 * Rb) + _align(8 * Rb)
    inst_gid = b[gid_off:gid_off + 4 * n_sorted].view(np.uint32).copy()
    nseg = Rb // 256 + 2
    lg_off = gid_off + _align(4 * Rb) + _align(48 * Rb) + _align(8 * nseg) + _align(nseg * 256 * 16)
    list_gid = b[lg_off:lg_off + 4 * n_sorted].view(np.uint32).copy()
    return dict(hdr=hdr[:9].copy(), sticky=hdr[60:61].copy(), log=np.array(log, dtype=np.int64), tiles=tiles, vis_list=vis_list,
                offsets=offsets, ranges=ranges, emission=emission, inst_gid=inst_gid, list_gid=list_gid, rec=rec,
                radii=radii.cpu().numpy(), color=color.cpu().numpy().view(np.uint32), depth=depth.cpu().numpy().view(np.uint32))


COMPARED = ("hdr", "log", "tiles", "vis_list", "offsets", "ranges", "emission", "inst_gid", "list_gid", "radii", "color", "depth")


def _runs(cloud, cam, dev, capacity=200_000, knobs=KNOBS, also=()):
    """The view under every knob value; all held to the first (the five launches).  Returns the default path's buffers."""
    P, w, h = cloud["means3D"].shape[0], cam.image_width, cam.image_height
    runs = {}
    for v in knobs:
        _lib.tune_set("bin_fuse", v)
        out, log = _forward(cloud, cam, dev, capacity)
        runs[v] = _unpack(out, log, P, w, h)
    _lib.tune_set("bin_fuse", -1)
    ref = runs[knobs[0]]
    for v in knobs[1:]:
        for k in COMPARED + tuple(also):
            assert np.array_equal(ref[k], runs[v][k]), (v, k)
    u = runs[knobs[-1]]
    # the lists of the scan are what they say: the emitting Gaussians in index order, their first slots the running sum
    emit = np.nonzero(u["tiles"])[0]
    assert np.array_equal(u["vis_list"], emit)
    assert np.array_equal(u["offsets"], np.concatenate([[0], np.cumsum(u["tiles"][emit])[:-1]]).astype(np.uint32))
    assert int(u["hdr"][8]) == emit.size and int(u["hdr"][6]) == int(u["tiles"].sum())
    assert list(u["log"][:8]) == [int(x) for x in u["hdr"][:8]]
    return u


def _splats(cam, tile_of, depth, w, h, seed=11):
    """One small isotropic splat per entry of tile_of, centred on its tile (the tile rectangle is that one tile), at the given view
    depth (identity camera: view depth == z); tile -1 = behind the camera (emits nothing)."""
    P = tile_of.shape[0]
    gx = (w + 15) // 16
    tfx, tfy = hp.tan_fov(cam)
    rng = np.random.default_rng(seed)
    t = np.maximum(tile_of, 0)
    px = (t % gx) * 16 + 8 + rng.integers(-3, 4, P)
    py = (t // gx) * 16 + 8 + rng.integers(-3, 4, P)
    z = depth.astype(np.float64)
    means = np.stack([((2 * px + 1) / w - 1) * z * tfx, ((2 * py + 1) / h - 1) * z * tfy, z], axis=1).astype(np.float32)
    means[tile_of < 0, 2] = -3.0
    shs = torch.zeros(P, 16, 3)
    shs[:, 0, :] = torch.from_numpy(rng.random((P, 3)).astype(np.float32))
    rot = torch.zeros(P, 4)
    rot[:, 0] = 1.0
    return dict(means3D=torch.from_numpy(means), scales=torch.full((P, 3), 1e-4), rotations=rot,
                opacities=torch.full((P, 1), 0.9), shs=shs)


def _assert_lists_are_the_lexsort(u, tile_of):
    """every tile's list: its Gaussians by (depth bits, index) -- the reference's stable 64-bit sort"""
    idx = np.arange(tile_of.shape[0])
    depth_bits = u["rec"][:, 9]
    point_list = u["inst_gid"][u["emission"]]
    assert np.array_equal(u["list_gid"], point_list)
    rng = u["ranges"].astype(np.int64)
    assert int((rng[:, 1] - rng[:, 0]).sum()) == int((tile_of >= 0).sum())
    for t in range(rng.shape[0]):
        mine = idx[tile_of == t]
        want = mine[np.lexsort((mine, depth_bits[mine]))]
        assert np.array_equal(point_list[rng[t, 0]:rng[t, 1]], want), t
        if mine.size == 0:
            assert rng[t, 0] == 0 and rng[t, 1] == 0


# ---- 1. bin sizes --------------------------------------------------------------------------------------------------------------
SMALL_AVERAGE = 256 * 12                        # capacity / tiles <= 256: the one-launch form of the per-bin sort


@pytest.mark.parametrize("capacity", [SMALL_AVERAGE, 200_000])
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65, 128, 129, 256, 257, 1025, 2049, 3000])
def test_one_tile_of_exactly_n(hip_device, n, ties, capacity):
    cam = cameras.identity_camera(W, H)
    rng = np.random.default_rng(100 * n + ties)
    tile_of = np.full(n, 6)                                     # the other eleven tiles stay empty
    if ties:
        depth = (3.0 + 0.25 * (rng.permutation(n) // 5)).astype(np.float32)      # groups of five at one depth: the slot decides
    else:
        depth = rng.permutation(np.linspace(2.0, 6.0, n, dtype=np.float32)).astype(np.float32)
    u = _runs(_splats(cam, tile_of, depth, W, H), cam, hip_device, capacity=capacity)
    assert int(u["hdr"][5]) == n and list(u["ranges"][6]) == [0, n]
    _assert_lists_are_the_lexsort(u, tile_of)


def test_three_queued_bins_beside_small_ones(hip_device):
    """Three tiles of a little more than 1024 entries (one, two and three depth values only: the slot decides nearly every
    comparison) beside small ones, in the one-launch form: the queue is strided over."""
    cam = cameras.identity_camera(W, H)
    rng = np.random.default_rng(21)
    counts = {0: 1025, 5: 1030, 11: 1010, 1: 1, 2: 2, 3: 0, 4: 1, 6: 0, 7: 1, 8: 0, 9: 1, 10: 0}
    assert sum(counts.values()) <= SMALL_AVERAGE
    tile_of = rng.permutation(np.concatenate([np.full(c, t) for t, c in counts.items()]))
    depth = rng.uniform(2.0, 6.0, tile_of.shape[0]).astype(np.float32)
    depth[tile_of == 0] = 4.0
    depth[tile_of == 5] = np.where(rng.random(1030) < 0.5, 3.0, 5.0).astype(np.float32)
    depth[tile_of == 11] = rng.choice(np.array([2.5, 3.5, 4.5], np.float32), 1010)
    u = _runs(_splats(cam, tile_of, depth, W, H), cam, hip_device, capacity=SMALL_AVERAGE)
    _assert_lists_are_the_lexsort(u, tile_of)


# ---- 2. overflow ---------------------------------------------------------------------------------------------------------------
def test_overflow_is_the_same_on_both_paths(hip_device):
    cam = cameras.identity_camera(W, H)
    rng = np.random.default_rng(2)
    P = 3000
    tile_of = rng.integers(0, 12, P)
    u = _runs(_splats(cam, tile_of, rng.uniform(2.0, 6.0, P).astype(np.float32), W, H), cam, hip_device, capacity=1000,
              also=("sticky",))               # (written only by a view that overflows, or the first of a step)
    overflow, capacity, n_sorted, n_inst = (int(u["hdr"][i]) for i in (1, 3, 5, 6))
    sticky = int(u["sticky"][0])
    assert (overflow, capacity, n_sorted, n_inst, sticky) == (1, 1000, 1000, P, 1)
    assert int(u["log"][1]) == 1 and int(u["log"][5]) == 1000 and int(u["log"][6]) == P
    rngs = u["ranges"].astype(np.int64)
    assert int((rngs[:, 1] - rngs[:, 0]).sum()) == 1000 and u["emission"].max() < 1000


# ---- 3. the multi-view step ----------------------------------------------------------------------------------------------------
N_STEP_VIEWS = 4


def _step(device, sc, train):
    from luciddreamer_amd import parallel
    P = sc["cloud"]["means3D"].shape[0]
    cams = sc["cams"][:N_STEP_VIEWS]
    w, h = cams[0].image_width, cams[0].image_height
    kw = dict(targets=sc["targets"][:N_STEP_VIEWS]) if train else {}
    batch = parallel.ViewBatch(cams, None if train else [sc["grad"]] * N_STEP_VIEWS, 3, sc["bg"], binning_capacity=200_000,
                               n_streams=3, **kw)
    colors = [torch.full((3, h, w), -1.0, device=device) for _ in range(N_STEP_VIEWS)]
    radii = [torch.full((P,), -1, dtype=torch.int32, device=device) for _ in range(N_STEP_VIEWS)]
    batch._args.out_color = _host_array(batch, colors)
    batch._args.out_radii = _host_array(batch, radii)
    acc = {k: torch.zeros((P,) + s, device=device) for k, s in ACC_SHAPES.items()}
    c = sc["cloud"]
    batch.run(c["means3D"], c["opacities"], c["scales"], c["rotations"], c["shs"], acc)
    batch.check()
    out = dict(acc)
    out["color"], out["radii"] = colors, radii
    if train:
        out["losses"] = batch.losses.clone()
    return out


@pytest.mark.parametrize("train", [False, True])
def test_multi_view_step_accumulates_the_same_bytes(hip_device, train):
    """Four views on three chains, with fixed upstream gradients and with targets; a second step gives the same bytes again."""
    sc = _step_scene(hip_device, "band")
    _lib.tune_set("bin_fuse", 0)
    want = _step(hip_device, sc, train)
    for v in (1, -1):
        _lib.tune_set("bin_fuse", v)
        first = _step(hip_device, sc, train)
        second = _step(hip_device, sc, train)
        _assert_same(first, want, f"bin_fuse={v}")
        _assert_same(second, want, f"bin_fuse={v}, second step")
    _lib.tune_set("bin_fuse", 0)
    _assert_same(_step(hip_device, sc, train), want, "back on the five launches")
    assert float(want["means3D"].abs().max()) > 0 and all(float(c.min()) >= 0 for c in want["color"])


# ---- 4. more than 16384 tiles --------------------------------------------------------------------------------------------------
def test_more_than_16384_tiles(hip_device):
    """2064 x 2048 = 129 x 128 tiles: a bin is two tiles and the per-bin sort writes the ranges."""
    w, h = 2064, 2048
    cam = cameras.identity_camera(w, h)
    rng = np.random.default_rng(4)
    P = 300
    tile_of = rng.integers(0, 129 * 128, P)
    tile_of[:40] = 2 * rng.integers(0, 8000, 1) + (np.arange(40) & 1)          # one bin with both of its tiles filled
    u = _runs(_splats(cam, tile_of, rng.uniform(2.0, 6.0, P).astype(np.float32), w, h), cam, hip_device)
    _assert_lists_are_the_lexsort(u, tile_of)


# ---- 5. both shapes of the blend forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [0, 2])
def test_forward_shapes(hip_device, shape):
    cam = cameras.identity_camera(W, H)
    rng = np.random.default_rng(8)
    tile_of = np.concatenate([np.full(c, t) for t, c in enumerate((0, 1, 60, 64, 100, 128, 129, 200, 300, 5, 0, 33))])
    tile_of = rng.permutation(tile_of)
    depth = rng.uniform(2.0, 6.0, tile_of.shape[0]).astype(np.float32)
    depth[::5] = 4.0
    _lib.tune_set("fwd_pair", shape)
    u = _runs(_splats(cam, tile_of, depth, W, H), cam, hip_device)
    _assert_lists_are_the_lexsort(u, tile_of)
