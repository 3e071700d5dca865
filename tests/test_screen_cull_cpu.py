"""CPU: the conservative off-screen test of the pooled preprocess kernel (csrc/screen_cull.h), compiled for the host with
-O2 -ffp-contract=off (the kernel's own float operations, bit for bit) and held against the oracle's radii.

Conservative: nothing the oracle gives a radius > 0 is ever rejected.  A Gaussian's radius does not depend on its neighbours,
so the oracle runs on the REJECTED rows only (none of them may come back with a radius) -- that keeps a 200 k cloud over
72 view / resolution / scale-modifier combinations within seconds -- and on the whole of the small built clouds.
Effective: on the bench's own scenes the test keeps at most 1.35 x what is visible among the near-plane passers."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from luciddreamer_amd import cameras, synthetic
from tests import helpers as hp

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "luciddreamer_amd", "csrc")

WRAPPER = r"""
#include <stdint.h>
#include "screen_cull.h"
// per row: bit 0 = passes the near plane (auxiliary.h:152-162), bit 1 = rejected by screen_cull_point
extern "C" void sc_run(int P, const float* means, const float* scales, const float* rots, const float* V, const float* Pm,
                       float scale_modifier, int W, int H, float tan_fovx, float tan_fovy, uint8_t* out)
{
    const int gx = (W + 15) / 16, gy = (H + 15) / 16;
    const float focal_y = H / (2.0f * tan_fovy), focal_x = W / (2.0f * tan_fovx);      // api.hip, where ViewParams is filled
    const lr::ScreenCull c = lr::screen_cull_view(W, H, gx, gy, tan_fovx, tan_fovy, focal_x, focal_y);
    const float kv9 = lr::screen_cull_kv9(c, V);
    for (int i = 0; i < P; i++) {
        const float x = means[3 * i], y = means[3 * i + 1], z = means[3 * i + 2];
        const float vz = V[2] * x + V[6] * y + V[10] * z + V[14];
        const bool near = !(vz <= 0.2f);
        const bool rej = lr::screen_cull_point(c, kv9, Pm, scale_modifier, x, y, z, vz, scales[3 * i], scales[3 * i + 1],
                                               scales[3 * i + 2], rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3]);
        out[i] = (uint8_t)((near ? 1 : 0) | (rej ? 2 : 0));
    }
}
"""


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / c++ / clang++) on this machine")
    d = tmp_path_factory.mktemp("screen_cull")
    src, so = d / "sc.cpp", d / "libsc.so"
    src.write_text(WRAPPER)
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.sc_run.restype, L.sc_run.argtypes = None, [ci, vp, vp, vp, vp, vp, cf, ci, ci, cf, cf, vp]

    def run(cloud, cam, scale_modifier=1.0):
        """(near, rejected) per row, as phase 1 of the pooled kernel decides them."""
        f = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        m, s, q = f(cloud["means3D"]), f(cloud["scales"]), f(cloud["rotations"])
        V, Pm = f(cam.world_view_transform).reshape(-1), f(cam.full_proj_transform).reshape(-1)
        out = np.zeros(m.shape[0], np.uint8)
        p = lambda a: a.ctypes.data_as(vp)
        tfx, tfy = hp.tan_fov(cam)
        L.sc_run(m.shape[0], p(m), p(s), p(q), p(V), p(Pm), scale_modifier, cam.image_width, cam.image_height, tfx, tfy, p(out))
        return (out & 1) != 0, (out & 2) != 0
    return run


BG = torch.zeros(3)


def _rows(cloud, rows):
    return {k: v[rows] for k, v in cloud.items()}


def _oracle_radii(cloud, cam, scale_modifier=1.0):
    return hp.run_oracle(cloud, cam, 0, BG, scale_modifier=scale_modifier)["radii"]


def _assert_conservative(sc, cloud, cam, scale_modifier=1.0, whole=False, what=""):
    """No row with an oracle radius is rejected.  Returns (near, rejected, oracle radii or None)."""
    near, rej = sc(cloud, cam, scale_modifier)
    radii = None
    if whole:
        radii = _oracle_radii(cloud, cam, scale_modifier)
        bad = np.nonzero(rej & near & (radii > 0))[0]
    else:
        rows = np.nonzero(rej & near)[0]
        bad = rows[_oracle_radii(_rows(cloud, torch.from_numpy(rows)), cam, scale_modifier) > 0] if rows.size else rows
    assert bad.size == 0, f"{what}: {bad.size} visible Gaussians rejected, first rows {bad[:8].tolist()}"
    return near, rej, radii


def _small_cloud(P, kind, seed=0):
    return synthetic.make_cloud(P, kind, seed, sh_coeffs=1)


@pytest.fixture(scope="module")
def clouds():
    return {kind: _small_cloud(200_000, kind) for kind in ("band", "shell")}


@pytest.mark.parametrize("kind", ["band", "shell"])
@pytest.mark.parametrize("res", [(1920, 1080), (512, 512)])
def test_conservative_on_the_bench_clouds(sc, clouds, kind, res):
    cloud = clouds[kind]
    path = cameras.rotate360_path(res[0], res[1], n_views=6)
    assert len(path) == 6
    for v, cam in enumerate(path):
        for mod in (0.5, 1.0, 3.0):
            near, rej, _ = _assert_conservative(sc, cloud, cam, mod, what=f"{kind} {res} view {v} modifier {mod}")
            assert (rej & near).sum() > 0.25 * near.sum()            # the test is not vacuous: it drops a good part of the passers


def _unproject(cam, px, py, z):
    """World points of an identity-view camera from pixel coordinates and depth."""
    tfx, tfy = hp.tan_fov(cam)
    W, H = cam.image_width, cam.image_height
    return np.stack([((2 * px + 1) / W - 1) * z * tfx, ((2 * py + 1) / H - 1) * z * tfy, z], axis=1).astype(np.float32)


def _unit_quats(P, rng):
    q = rng.standard_normal((P, 4))
    return torch.from_numpy((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32))


def edge_cloud(cam, rng):
    """Splats just outside each of the four sides and four corners of the screen: the centre d pixels outside, d swept in
    steps of half a pixel over radius - 4 .. radius + 4 for splats of about 3 / 8 / 20 / 60 pixels in radius, so that
    radius - d takes every value of -2, -1, 0, 1, 2 (and the halves between) on every side; and per size two splats far
    out (4 and 8 radii), which the bound -- about 3 x the radius for a round splat -- must reject.  Returns the cloud and
    per row (side, d, far)."""
    W, H = cam.image_width, cam.image_height
    focal = W / (2 * hp.tan_fov(cam)[0])
    px, py, sig, side, dist, far = [], [], [], [], [], []
    for sx, sy in [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]:
        for r_est in (3, 8, 20, 60):
            for d in list(np.arange(max(r_est - 4.0, 0.0), r_est + 4.25, 0.5)) + [4.0 * r_est + 12.0, 8.0 * r_est + 30.0]:
                # pixel centres: -d is d pixels left of pixel 0; 16 gx - 1 + d is d pixels right of the tile grid's last one
                x = rng.uniform(20, W - 20) if sx == 0 else (-d if sx < 0 else 16 * ((W + 15) // 16) - 1 + d)
                y = rng.uniform(20, H - 20) if sy == 0 else (-d if sy < 0 else 16 * ((H + 15) // 16) - 1 + d)
                px.append(x); py.append(y); side.append((sx, sy)); dist.append(d); far.append(d > r_est + 5.0)
                sig.append(math.sqrt(max(((r_est - 0.5) / 3.0) ** 2 - 0.3, 1e-6)))            # radius = ceil(3 sqrt(sigma^2 + 0.3))
    P = len(px)
    z = np.full(P, 4.0)
    s = (np.array(sig) * 4.0 / focal).astype(np.float32)
    scales = np.stack([s, s, 1e-3 * s], axis=1)                    # discs in the image plane: the radius holds off-axis too
    q = torch.zeros(P, 4); q[:, 0] = 1.0
    cloud = dict(means3D=torch.from_numpy(_unproject(cam, np.array(px), np.array(py), z)), scales=torch.from_numpy(scales),
                 rotations=q, opacities=torch.full((P, 1), 0.5), shs=torch.zeros(P, 1, 3))
    return cloud, side, np.array(dist), np.array(far)


@pytest.mark.parametrize("res", [(1920, 1080), (512, 512), (250, 130)])
def test_conservative_on_the_edge(sc, res):
    cam = cameras.identity_camera(*res)
    cloud, side, d, far = edge_cloud(cam, np.random.default_rng(3))
    near, rej, radii = _assert_conservative(sc, cloud, cam, whole=True, what=f"edge cloud {res}")
    assert near.all()
    side = np.array(side)
    for s in np.unique(side, axis=0):
        rows = (side == s).all(axis=1) & ~far
        k = np.round(radii[rows] - d[rows]).astype(int)
        vis = radii[rows] > 0
        assert vis.any() and (~vis).any(), f"side {s}: the sweep must straddle the edge"
        # d moves in half pixels, so a sweep that straddles the edge holds every radius - d around it; the last visible one
        # has radius - d = 1 on the left (pix + radius + 15 >= 16) and -1 on the right (pix - radius < 16 gx), give or take
        # the rounding of pix; a corner needs both axes
        assert -1 <= k[vis].min() <= 2, (s, sorted(set(k[vis].tolist())))
    assert rej[far].all() and (radii[far] == 0).all()


def test_conservative_near_plane_far_off_axis(sc):
    """vz in (0.2, 0.25], |vx / vz| far beyond the 1.3 tan clamp, large scales: the Jacobian is at its clamp, the radius in
    the hundreds or thousands of pixels."""
    rng = np.random.default_rng(5)
    P = 20_000
    for res in ((1920, 1080), (512, 512)):
        cam = cameras.identity_camera(*res)
        tfx, tfy = hp.tan_fov(cam)
        z = rng.uniform(0.2001, 0.25, P)
        rx = rng.uniform(1.5, 60.0, P) * rng.choice([-1, 1], P) * tfx
        ry = rng.uniform(0.0, 60.0, P) * rng.choice([-1, 1], P) * tfy
        means = np.stack([rx * z, ry * z, z], axis=1).astype(np.float32)
        scales = np.exp(rng.uniform(math.log(1e-3), math.log(2.0), (P, 3))).astype(np.float32)
        cloud = dict(means3D=torch.from_numpy(means), scales=torch.from_numpy(scales), rotations=_unit_quats(P, rng),
                     opacities=torch.full((P, 1), 0.5), shs=torch.zeros(P, 1, 3))
        near, rej, _ = _assert_conservative(sc, cloud, cam, what=f"near plane {res}")
        assert near.all() and rej.sum() > 1000
        # a small part through the whole oracle: the scene does hold splats that reach the screen from out there
        _, _, radii = _assert_conservative(sc, _rows(cloud, slice(0, 1000)), cam, whole=True, what=f"near plane {res}")
        assert (radii > 0).sum() > 50


def _diag_quat(P):
    q = torch.zeros(P, 4)
    q[:, 0], q[:, 3] = math.cos(math.pi / 8), math.sin(math.pi / 8)      # 45 degrees about the view axis
    return q


def test_conservative_thin_diagonal_splats(sc):
    """Anisotropy 1 : 100 at 45 degrees, centres up to two screens away."""
    rng = np.random.default_rng(6)
    P = 30_000
    cam = cameras.identity_camera(512, 512)
    focal = 512 / (2 * hp.tan_fov(cam)[0])
    z = rng.uniform(1.0, 6.0, P)
    px, py = rng.uniform(-1024, 1536, P), rng.uniform(-1024, 1536, P)
    major = np.exp(rng.uniform(math.log(1.0), math.log(600.0), P)) * z / focal          # sigma of 1 .. 600 pixels
    scales = np.stack([major, 0.01 * major, 0.01 * major], axis=1).astype(np.float32)
    cloud = dict(means3D=torch.from_numpy(_unproject(cam, px, py, z)), scales=torch.from_numpy(scales), rotations=_diag_quat(P),
                 opacities=torch.full((P, 1), 0.5), shs=torch.zeros(P, 1, 3))
    near, rej, _ = _assert_conservative(sc, cloud, cam, what="thin diagonal splats")
    assert rej.sum() > 3000
    _, _, radii = _assert_conservative(sc, _rows(cloud, slice(0, 1500)), cam, whole=True, what="thin diagonal splats")
    assert (radii > 0).sum() > 150


@pytest.mark.parametrize("norm", [0.5, 1.0, 2.0])
def test_conservative_with_quaternions_of_any_norm(sc, clouds, norm):
    """The chain uses the quaternion as given: R(q) of a non-unit q stretches (|q| = 2: up to 7 x) or squashes."""
    cloud = dict(clouds["band"])
    cloud = _rows(cloud, slice(0, 60_000))
    cloud["rotations"] = cloud["rotations"] * norm
    for res in ((1920, 1080), (512, 512)):
        for cam in cameras.rotate360_path(res[0], res[1], n_views=3):
            for mod in (1.0, 3.0):
                near, rej, _ = _assert_conservative(sc, cloud, cam, mod, what=f"|q| = {norm} {res}")
                assert rej.sum() > 1000


def posed_camera(W, H):
    """Translation, pitch and roll (and some yaw): nothing about the view is axis-aligned."""
    def rot(axis, deg):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        i, j = [(1, 2), (0, 2), (0, 1)][axis]
        R = np.eye(3); R[i, i] = c; R[j, j] = c; R[i, j] = -s; R[j, i] = s
        return R
    c2w = np.eye(4)
    c2w[:3, :3] = rot(1, 25.0) @ rot(0, 20.0) @ rot(2, 30.0)
    c2w[:3, 3] = [0.4, -0.3, 0.6]
    return cameras.make_camera(c2w, W, H)


@pytest.mark.parametrize("res", [(1920, 1080), (512, 512)])
def test_conservative_for_a_posed_camera(sc, clouds, res):
    cam = posed_camera(*res)
    for kind in ("band", "shell"):
        for mod in (0.5, 1.0, 3.0):
            near, rej, _ = _assert_conservative(sc, clouds[kind], cam, mod, what=f"posed camera {kind} {res} modifier {mod}")
            assert (rej & near).sum() > 0.25 * near.sum()
    # ... and its own edge: the edge cloud of the identity view carried into this camera's frame
    ident = cameras.identity_camera(*res)
    cloud, _, _, far = edge_cloud(ident, np.random.default_rng(4))
    c2w = torch.inverse(cam.world_view_transform.T.double())
    cloud["means3D"] = (cloud["means3D"].double() @ c2w[:3, :3].T + c2w[:3, 3]).float()
    near, rej, radii = _assert_conservative(sc, cloud, cam, whole=True, what=f"posed edge cloud {res}")
    assert (radii > 0).any() and rej[far].all()


@pytest.mark.parametrize("case", ["wide", "narrow", "tall_pixels", "wide_pixels", "off_centre", "general"])
def test_conservative_under_general_intrinsics(sc, case):
    """The six rows of tests/intrinsics_cases.py (focal_x != focal_y, a shifted principal point, wide and narrow fields of view),
    each on its own cloud, and on the band cloud, of which every row sees a part only."""
    from tests import intrinsics_cases as ic
    assert case in ic.CASES and len(ic.CASES) == 6
    cam, cloud, _ = ic.make(case)
    near, rej, radii = _assert_conservative(sc, cloud, cam, whole=True, what=case)
    assert (radii > 0).sum() >= 0.4 * radii.size and (rej & near).sum() > 0
    band = _small_cloud(20_000, "band", 1)
    for mod in (1.0, 3.0):
        near, rej, _ = _assert_conservative(sc, band, cam, mod, what=f"{case} band modifier {mod}")
        assert (rej & near).sum() > 0


def test_rows_that_are_no_numbers_pass(sc, clouds):
    """NaN / inf / 0 / negative scales, NaN and inf means, NaN quaternions: the test must let them through (NaN, inf) or
    stay conservative (0, negative: |scale| is what the covariance sees)."""
    cam = cameras.rotate360_path(512, 512, n_views=6)[1]
    cloud = {k: v.clone() for k, v in _rows(clouds["band"], slice(0, 40_000)).items()}
    near0, rej0 = sc(cloud, cam)
    rows = torch.from_numpy(np.nonzero(near0 & rej0)[0][:6000])          # rows the test rejects as they are
    assert rows.numel() == 6000
    nan, inf = float("nan"), float("inf")
    g = [rows[i::10] for i in range(10)]
    cloud["scales"][g[0], 0] = nan; cloud["scales"][g[1], 1] = nan; cloud["scales"][g[2], 2] = nan
    cloud["scales"][g[3], 1] = inf; cloud["scales"][g[4], 2] = -inf
    cloud["means3D"][g[5], 0] = nan; cloud["means3D"][g[6], 2] = nan
    cloud["rotations"][g[7], 2] = nan
    cloud["scales"][g[8]] = 0.0
    cloud["scales"][g[9]] *= -1.0
    near, rej = sc(cloud, cam)
    for i in range(8):
        assert not rej[g[i].numpy()].any(), f"group {i}: a row without a number was rejected"
    assert rej[g[8].numpy()].all() and rej[g[9].numpy()].all()          # 0 and negative scales are numbers: still rejected ...
    finite = torch.cat([g[8], g[9]])
    assert (_oracle_radii(_rows(cloud, finite), cam) == 0).all()        # ... and rightly so


# kept <= 1.35 x visible among the near-plane passers: what makes the test worth its cost in phase 1 (a bound that keeps
# more has a mistake in it).  The bench's own scenes, all 1 M rows through the test; the oracle on a 100 k row sample.
@pytest.mark.parametrize("kind,res,views", [("band", (1920, 1080), (0, 7, 19)), ("shell", (512, 512), (0, 11))])
def test_effective_on_the_bench_scenes(sc, kind, res, views):
    cloud = _small_cloud(1_000_000, kind)
    path = cameras.rotate360_path(res[0], res[1], n_views=30)
    sample = torch.from_numpy(np.sort(np.random.default_rng(1).permutation(1_000_000)[:100_000]))
    sub = _rows(cloud, sample)
    for v in views:
        near, rej = sc(cloud, path[v])
        radii = _oracle_radii(sub, path[v])
        s = sample.numpy()
        visible = int((radii > 0).sum())
        kept = int((near[s] & ~rej[s]).sum())
        assert not (rej[s] & (radii > 0)).any()
        ratio = kept / visible
        print(f"{kind} {res} view {v}: near {int(near.sum())} kept {int((near & ~rej).sum())} of 1 M; sample: kept {kept} visible {visible} "
              f"ratio {ratio:.3f}")
        assert visible > 5000 and ratio <= 1.35, (kind, v, kept, visible)
