"""GPU: the per-bin rank sort of k_tile_sort_small (lr_tune_set("tsort", 3)) writes the same lists and ranges, bit for bit,
as the bucket sort / bitonic network it replaces ("tsort" 2 and 0) -- and as a lexsort of (depth bits, Gaussian index) per tile,
which is what the reference's stable 64-bit sort produces.  Scenes are built so that one tile receives EXACTLY n instances
(sizes around every boundary of the per-bin algorithms: one / two / four words per lane, the wave-sized limit of 256) under
four depth patterns, plus one image of more than 16384 tiles, where a bin holds two tiles and the sort writes the ranges."""
import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, cameras
from tests import helpers as hp

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 128, 255, 256, 257]
PATTERNS = ["random", "equal", "pairs", "descending"]
KNOBS = [3, 2, 0, -1, 4]                  # rank sort, bucket sort + network, network only, the default rule, rank sort up to 128


@pytest.fixture(autouse=True)
def _restore_knob():
    yield
    _lib.tune_set("tsort", -1)


def _align(n):
    return (n + 255) // 256 * 256


def _depths(pattern, n, rng):
    if pattern == "random":
        return rng.permutation(np.linspace(2.0, 6.0, n, dtype=np.float32)).astype(np.float32)
    if pattern == "equal":
        return np.full(n, 4.0, np.float32)
    if pattern == "pairs":
        return (3.0 + 0.01 * (np.arange(n) // 2)).astype(np.float32)
    return (6.0 - 0.005 * np.arange(n)).astype(np.float32)            # strictly descending with the index


def _scene(cam, tile_of, depth, W, H):
    """One small isotropic splat per entry of tile_of, centred on its tile (3-sigma radius 2 px: the tile rectangle is that
    one tile), at the given view depth (identity camera: view depth == z)."""
    P = tile_of.shape[0]
    gx = (W + 15) // 16
    tfx, tfy = hp.tan_fov(cam)
    rng = np.random.default_rng(11)
    px = (tile_of % gx) * 16 + 8 + rng.integers(-3, 4, P)
    py = (tile_of // gx) * 16 + 8 + rng.integers(-3, 4, P)
    z = depth.astype(np.float64)
    means = np.stack([((2 * px + 1) / W - 1) * z * tfx, ((2 * py + 1) / H - 1) * z * tfy, z], axis=1).astype(np.float32)
    shs = torch.zeros(P, 16, 3)
    shs[:, 0, :] = torch.from_numpy(rng.random((P, 3)).astype(np.float32))
    rot = torch.zeros(P, 4)
    rot[:, 0] = 1.0
    return dict(means3D=torch.from_numpy(means), scales=torch.full((P, 3), 1e-4), rotations=rot,
                opacities=torch.full((P, 1), 0.9), shs=shs)


def _forward(cloud, cam, dev):
    from luciddreamer_amd import _C
    tfx, tfy = hp.tan_fov(cam)
    c = cam.to(dev)
    e = torch.Tensor([])
    return _C.rasterize_gaussians(torch.zeros(3, device=dev), cloud["means3D"].to(dev), e, cloud["opacities"].to(dev),
                                  cloud["scales"].to(dev), cloud["rotations"].to(dev), 1.0, e, c.world_view_transform,
                                  c.full_proj_transform, tfx, tfy, cam.image_height, cam.image_width,
                                  cloud["shs"].to(dev), 3, c.camera_center, False, False, binning_capacity=0)


def _unpack(out, P, W, H):
    """csrc/common.h geom / img / bin layouts, as tests/test_gpu_full.py reads them, plus list_gid (the Gaussian of every list
    position, which the per-bin sort writes next to the list)."""
    num_rendered, color, depth, radii, geom, binning, img = out
    g = geom.cpu().numpy()
    hdr = g[:32].view(np.uint32)
    rec = g[256:256 + 48 * P].view(np.float32).reshape(P, 12)
    N, T = W * H, ((W + 15) // 16) * ((H + 15) // 16)
    im = img.cpu().numpy()
    ranges = im[2 * _align(4 * N):2 * _align(4 * N) + 8 * T].view(np.uint32).reshape(T, 2).copy()
    n_inst = int(hdr[5])
    b = binning.cpu().numpy()
    emission = b[:4 * n_inst].view(np.uint32).copy()
    Rb = max(int(hdr[7]), 1)
    gid_off = _align(4 * Rb) + _align(8 * Rb)
    inst_gid = b[gid_off:gid_off + 4 * Rb].view(np.uint32)
    nseg = Rb // 256 + 2
    lg_off = gid_off + _align(4 * Rb) + _align(48 * Rb) + _align(8 * nseg) + _align(nseg * 256 * 16)
    list_gid = b[lg_off:lg_off + 4 * n_inst].view(np.uint32).copy()
    return dict(ranges=ranges, emission=emission, point_list=inst_gid[emission], list_gid=list_gid, depth_bits=rec[:, 9].copy().view(np.uint32),
                color=color.cpu().numpy(), depth=depth.cpu().numpy(), n_inst=n_inst)


def _check(cloud, cam, tile_of, W, H, dev):
    P = tile_of.shape[0]
    runs = {}
    for v in KNOBS:
        _lib.tune_set("tsort", v)
        runs[v] = _unpack(_forward(cloud, cam, dev), P, W, H)
    _lib.tune_set("tsort", -1)
    ref = runs[3]
    assert ref["n_inst"] == P                                  # every splat lands on exactly its one tile
    for v in KNOBS[1:]:
        for k in ("ranges", "emission", "list_gid", "color", "depth"):
            assert np.array_equal(ref[k], runs[v][k]), (v, k)
    idx = np.arange(P)
    for v in (3, -1, 4):
        u = runs[v]
        assert np.array_equal(u["list_gid"], u["point_list"])
        rng = u["ranges"].astype(np.int64)
        assert int((rng[:, 1] - rng[:, 0]).sum()) == P
        for t in range(rng.shape[0]):
            mine = idx[tile_of == t]
            want = mine[np.lexsort((mine, u["depth_bits"][mine]))]
            assert np.array_equal(u["point_list"][rng[t, 0]:rng[t, 1]], want), (v, t)
            if mine.size == 0:
                assert rng[t, 0] == 0 and rng[t, 1] == 0
    return runs


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_one_tile_of_exactly_n(hip_device, n, pattern):
    W = H = 32
    cam = cameras.identity_camera(W, H)
    counts = {3: n, 0: 7, 1: 70, 2: 150}                        # the tile under test and three other size classes beside it
    tile_of = np.concatenate([np.full(c, t) for t, c in counts.items()])
    rng = np.random.default_rng(1000 * n + PATTERNS.index(pattern))
    tile_of = rng.permutation(tile_of)                          # Gaussian indices interleave between the tiles
    depth = np.empty(tile_of.shape[0], np.float32)
    for t in counts:
        sel = np.nonzero(tile_of == t)[0]                       # ascending index: "descending" means with the index
        depth[sel] = _depths(pattern, sel.size, rng)
    _check(_scene(cam, tile_of, depth, W, H), cam, tile_of, W, H, hip_device)


def test_bins_of_two_tiles_write_their_ranges(hip_device):
    """129 x 129 = 16641 tiles: a bin is two consecutive tiles (sub_shift 1) and the per-bin sort writes the ranges.  Bins with
    both tiles filled (the first tile's run starts the bin, the second one's ends it), with only one of them, and of every
    words-per-lane class of the rank sort."""
    W = H = 129 * 16
    cam = cameras.identity_camera(W, H)
    pairs = {40: (10, 20), 777: (0, 33), 1500: (40, 0), 4000: (50, 60), 6001: (100, 90), 8000: (1, 1), 8320: (3, 0), 0: (0, 5), 5123: (130, 2)}
    tile_of = np.concatenate([np.full(c, 2 * b + s) for b, cs in pairs.items() for s, c in enumerate(cs)])
    assert tile_of.max() < 129 * 129
    rng = np.random.default_rng(5)
    tile_of = rng.permutation(tile_of)
    depth = _depths("random", tile_of.shape[0], rng)
    depth[::7] = 4.0                                            # some ties inside and across the tiles
    _check(_scene(cam, tile_of, depth, W, H), cam, tile_of, W, H, hip_device)


def test_two_runs_of_one_view_give_identical_buffers(hip_device):
    W = H = 32
    cam = cameras.identity_camera(W, H)
    rng = np.random.default_rng(3)
    tile_of = rng.permutation(np.concatenate([np.full(c, t) for t, c in enumerate((50, 64, 100, 200))]))
    cloud = _scene(cam, tile_of, _depths("pairs", tile_of.shape[0], rng), W, H)
    a = _unpack(_forward(cloud, cam, hip_device), tile_of.shape[0], W, H)
    b = _unpack(_forward(cloud, cam, hip_device), tile_of.shape[0], W, H)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
