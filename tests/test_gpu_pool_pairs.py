"""GPU: the pooled preprocess kernel (lr_tune_set("preprocess", 1)) against the thread-per-Gaussian kernel ("preprocess", 0),
which is its bit-exact reference: radii, instance counts, the tile masks of the binning's HitRec, the records, the lists and
the images are IDENTICAL.  The scenes aim at phase 3b of the pooled kernel -- the exact tile test with one (Gaussian, tile)
pair per thread, its owner found in the pool's prefix of test counts: pools with 0 / 1 / 255 / 256 / 257 / 512 survivors, a cloud that ends in
the middle of a pool, rectangles on both sides of the 64-tile mask limit and of the 96-tile culling limit (thin diagonal
splats: part of every rectangle is culled), conics that are no proper ellipse, and opacities that can never reach 1/255."""
import math

import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, cameras
from tests import helpers as hp

pytestmark = pytest.mark.gpu

AREAS = [1, 2, 63, 64, 65, 96, 97]


@pytest.fixture(autouse=True)
def _restore_knob():
    yield
    _lib.tune_set("preprocess", -1)


def _align(n):
    return (n + 255) // 256 * 256


def _forward(cloud, cam, dev):
    from luciddreamer_amd import _C
    tfx, tfy = hp.tan_fov(cam)
    c = cam.to(dev)
    e = torch.Tensor([])
    cov = cloud.get("cov3D")
    return _C.rasterize_gaussians(torch.zeros(3, device=dev), cloud["means3D"].to(dev), e, cloud["opacities"].to(dev),
                                  e if cov is not None else cloud["scales"].to(dev), e if cov is not None else cloud["rotations"].to(dev),
                                  1.0, cov.to(dev) if cov is not None else e, c.world_view_transform,
                                  c.full_proj_transform, tfx, tfy, cam.image_height, cam.image_width,
                                  cloud["shs"].to(dev), 3, c.camera_center, False, False, binning_capacity=0)


def _unpack(out, P, W, H):
    """csrc/common.h geom / img / bin layouts (as tests/test_gpu_full.py reads them), with the per-Gaussian planes of the geom
    buffer: header, records, clamped, tiles_touched, vis_list, offsets, HitRec."""
    num_rendered, color, depth, radii, geom, binning, img = out
    g = geom.cpu().numpy()
    hdr = g[:48].view(np.uint32).copy()
    o = 256
    rec = g[o:o + 48 * P].view(np.uint32).reshape(P, 12).copy(); o += _align(48 * P)
    clamped = g[o:o + P].copy(); o += _align(P)
    tiles = g[o:o + 4 * P].view(np.uint32).copy(); o += 3 * _align(4 * P)
    hitrec = g[o:o + 16 * P].view(np.uint32).reshape(P, 4).copy()
    N, T = W * H, ((W + 15) // 16) * ((H + 15) // 16)
    im = img.cpu().numpy()
    ranges = im[2 * _align(4 * N):2 * _align(4 * N) + 8 * T].view(np.uint32).reshape(T, 2).copy()
    n_inst = int(hdr[5])
    b = binning.cpu().numpy()
    emission = b[:4 * n_inst].view(np.uint32).copy()
    Rb = max(int(hdr[7]), 1)
    gid_off = _align(4 * Rb) + _align(8 * Rb)
    inst_gid = b[gid_off:gid_off + 4 * n_inst].view(np.uint32).copy()
    return dict(num_rendered=num_rendered, hdr=hdr[:9], rec=rec, clamped=clamped, tiles=tiles, hitrec=hitrec, ranges=ranges,
                emission=emission, inst_gid=inst_gid, radii=radii.cpu().numpy(), color=color.cpu().numpy().view(np.uint32), depth=depth.cpu().numpy().view(np.uint32))


def _compare(cloud, cam, dev):
    """Both kernels on one scene; returns the pooled kernel's buffers."""
    P, W, H = cloud["means3D"].shape[0], cam.image_width, cam.image_height
    runs = []
    for v in (0, 1):
        _lib.tune_set("preprocess", v)
        runs.append(_unpack(_forward(cloud, cam, dev), P, W, H))
    _lib.tune_set("preprocess", -1)
    a, b = runs
    assert a["num_rendered"] == b["num_rendered"]
    for k in ("hdr", "radii", "tiles", "ranges", "emission", "inst_gid", "color", "depth"):
        assert np.array_equal(a[k], b[k]), k
    vis = a["radii"] > 0                                       # records and clamp bits exist for these only
    assert np.array_equal(a["rec"][vis], b["rec"][vis]) and np.array_equal(a["clamped"][vis], b["clamped"][vis])
    emit = a["tiles"] != 0                                     # the binning's record is read for the emitting ones only
    assert np.array_equal(a["hitrec"][emit], b["hitrec"][emit])
    return b


def _rect_areas(u, W, H):
    """Tile-rectangle area of every visible Gaussian, from its record (pixel centre) and radius: auxiliary.h getRect in float32."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rec = u["rec"].view(np.float32)
    px, py, r = rec[:, 0], rec[:, 1], u["radii"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        x0 = np.clip(((px - r) / np.float32(16)).astype(np.int64), 0, gx); x1 = np.clip(((px + r + np.float32(15)) / np.float32(16)).astype(np.int64), 0, gx)
        y0 = np.clip(((py - r) / np.float32(16)).astype(np.int64), 0, gy); y1 = np.clip(((py + r + np.float32(15)) / np.float32(16)).astype(np.int64), 0, gy)
    return np.where(u["radii"] > 0, (x1 - x0) * (y1 - y0), 0)


def _diag_quat(P):
    q = torch.zeros(P, 4)
    q[:, 0], q[:, 3] = math.cos(math.pi / 8), math.sin(math.pi / 8)      # 45 degrees about the view axis
    return q


def _unproject(cam, px, py, z):
    tfx, tfy = hp.tan_fov(cam)
    W, H = cam.image_width, cam.image_height
    return np.stack([((2 * px + 1) / W - 1) * z * tfx, ((2 * py + 1) / H - 1) * z * tfy, z], axis=1).astype(np.float32)


def _shs(P, rng):
    shs = torch.zeros(P, 16, 3)
    shs[:, 0, :] = torch.from_numpy(rng.random((P, 3)).astype(np.float32))
    shs[:, 1:, :] = torch.from_numpy((0.1 * rng.standard_normal((P, 15, 3))).astype(np.float32))
    return shs


def _pool_scene(cam, survivors, tail, rng):
    """Pools of 512 consecutive Gaussians with the given numbers of survivors (near plane passed, tile rectangle not empty),
    then `tail` more Gaussians (a last, partial pool).  The others fall behind the near plane or off the screen.  Survivors are
    thin splats along the diagonal, 2 to 60 pixels in radius, so that the exact tile test keeps part of a rectangle."""
    W, H = cam.image_width, cam.image_height
    counts = list(survivors) + [tail // 2]
    sizes = [512] * len(survivors) + [tail]
    P = sum(sizes)
    alive = np.zeros(P, bool)
    o = 0
    for c, n in zip(counts, sizes):
        alive[o + rng.permutation(n)[:c]] = True
        o += n
    z = rng.uniform(2.0, 6.0, P)
    px, py = rng.uniform(4, W - 4, P), rng.uniform(4, H - 4, P)
    dead = np.nonzero(~alive)[0]
    z[dead[0::2]] = -1.0                                        # phase 1 drops these
    px[dead[1::2]] = 40.0 * W                                   # phase 2 drops these: empty rectangle
    focal = W / (2 * hp.tan_fov(cam)[0])
    major = rng.uniform(0.4, 20.0, P) * z.clip(0.5) / focal     # 3 sigma of 1.2 .. 60 pixels
    scales = np.stack([major, 0.02 * major, 0.02 * major], axis=1).astype(np.float32)
    opac = rng.uniform(0.02, 1.0, (P, 1)).astype(np.float32)
    opac[rng.permutation(P)[:P // 20]] = 0.0                    # can never reach 1/255: every tile dropped
    opac[rng.permutation(P)[:P // 20]] = -0.25
    return dict(means3D=torch.from_numpy(_unproject(cam, px, py, z)), scales=torch.from_numpy(scales), rotations=_diag_quat(P),
                opacities=torch.from_numpy(opac), shs=_shs(P, rng)), alive


def test_pools_of_every_fill(hip_device):
    cam = cameras.identity_camera(256, 256)
    rng = np.random.default_rng(7)
    survivors = [0, 1, 255, 256, 257, 512]
    cloud, alive = _pool_scene(cam, survivors, 300, rng)       # 6 * 512 + 300 Gaussians: not a multiple of the pool
    u = _compare(cloud, cam, hip_device)
    got = [(u["radii"][512 * k:512 * (k + 1)] > 0).sum() for k in range(len(survivors))]
    assert got == survivors, got                                # the pools hold what the scene was built for
    assert (u["radii"][512 * len(survivors):] > 0).sum() == 150
    assert 0 < (u["tiles"] != 0).sum() < alive.sum()            # opacity <= 0: survivors that emit nothing
    areas = _rect_areas(u, 256, 256)
    culled = (u["tiles"] != 0) & (u["tiles"] < areas) & (areas <= 96)
    assert culled.sum() > 100                                   # rectangles only partly kept by the tile test


def test_rectangle_areas_around_the_mask_and_culling_limits(hip_device):
    """One row of 100 tiles: a rectangle is n x 1, so every area can be made, 97 (a prime) included.  Per area a thin diagonal
    splat (most of the row culled, 97 emitted whole), a round one (all kept) and one with opacity 0 (only the tile its centre
    lies in is kept: that one passes without a test)."""
    W, H = 1600, 16
    cam = cameras.identity_camera(W, H)
    rng = np.random.default_rng(9)
    focal = W / (2 * hp.tan_fov(cam)[0])
    px, major, minor, opac = [], [], [], []
    for n in AREAS:
        r = max(3, 8 * n - 7)                                   # px - r = 16 a + 0.5, px + r + 15 = 16 (a + n) + 1.5
        # pixels: radius = ceil(3 sqrt(s^2 + 0.3)) = r; the smallest radius there is, 3 (forward.cu:229-232 floors the
        # eigenvalue gap at sqrt(0.1)), for the one-tile rectangle
        s = math.sqrt(((r - 0.5) / 3.0) ** 2 - 0.3) if n > 1 else 1e-3
        for kind in range(3):
            px.append(16.0 + r + 0.5); major.append(s); minor.append(s if kind == 1 else 0.01 * s); opac.append(0.0 if kind == 2 else 0.8)
    flat = [1e-3 * m for m in major]                            # discs in the image plane: no depth extent, the radius is exact off-axis too
    P = len(px)
    z = np.full(P, 4.0)
    scales = (np.stack([major, minor, flat], axis=1) * 4.0 / focal).astype(np.float32)
    cloud = dict(means3D=torch.from_numpy(_unproject(cam, np.array(px), np.full(P, 8.0), z)), scales=torch.from_numpy(scales),
                 rotations=_diag_quat(P), opacities=torch.tensor(opac).reshape(P, 1), shs=_shs(P, rng))
    u = _compare(cloud, cam, hip_device)
    areas = _rect_areas(u, W, H)
    assert list(areas) == [n for n in AREAS for _ in range(3)], list(areas)
    tiles = u["tiles"].reshape(len(AREAS), 3)
    for i, n in enumerate(AREAS):
        if n <= 96:
            assert 0 < tiles[i, 0] <= n and tiles[i, 1] == n and tiles[i, 2] == 1
            assert n < 8 or tiles[i, 0] < n                     # the thin splat leaves most of a long row
        else:
            assert tiles[i, 0] == n and tiles[i, 1] == n and tiles[i, 2] == n      # beyond the limit: emitted unculled
    geo = u["hitrec"][:, 2].reshape(len(AREAS), 3)
    for i, n in enumerate(AREAS):
        assert (geo[i, :2] != 0).all() == (n <= 64)             # a mask up to 64 tiles, none beyond


def no_ellipse_scene():
    """(cam, cloud) with precomputed 3D covariances, a third of them indefinite (tests/test_gauss_project_cpu.py runs the
    same rows through the host build of the projection chain)."""
    W = H = 256
    cam = cameras.identity_camera(W, H)
    rng = np.random.default_rng(13)
    P = 1500
    focal = W / (2 * hp.tan_fov(cam)[0])
    z = rng.uniform(2.0, 6.0, P)
    sig = rng.uniform(0.5, 8.0, (P, 3)) * (z / focal)[:, None]
    var = sig ** 2
    odd = rng.permutation(P)[:P // 3]
    var[odd, 0] *= -1.0                                         # x variance negative: no ellipse
    cov = np.zeros((P, 6), np.float32)
    cov[:, 0], cov[:, 3], cov[:, 5] = var[:, 0], var[:, 1], var[:, 2]
    cov[:, 1] = 0.3 * np.sqrt(np.abs(var[:, 0] * var[:, 1])) * rng.uniform(-1, 1, P)
    opac = rng.uniform(0.02, 1.0, (P, 1)).astype(np.float32)
    cloud = dict(means3D=torch.from_numpy(_unproject(cam, rng.uniform(4, W - 4, P), rng.uniform(4, H - 4, P), z)),
                 cov3D=torch.from_numpy(cov), opacities=torch.from_numpy(opac), shs=_shs(P, rng))
    return cam, cloud


def test_conics_that_are_no_ellipse(hip_device):
    """Precomputed 3D covariances, some of them indefinite: the screen-space covariance then has a negative determinant, the
    conic a non-positive diagonal, and the tile test keeps every tile of the rectangle ("not a proper ellipse")."""
    cam, cloud = no_ellipse_scene()
    W = H = 256
    u = _compare(cloud, cam, hip_device)
    rec = u["rec"].view(np.float32)
    improper = (u["radii"] > 0) & ~((rec[:, 2] > 0) & (rec[:, 4] > 0))
    assert improper.sum() > 100
    areas = _rect_areas(u, W, H)
    assert np.array_equal(u["tiles"][improper], areas[improper])     # kept whole
