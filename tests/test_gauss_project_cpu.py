"""CPU: the per-Gaussian projection chain of both preprocess kernels (csrc/gauss_project.h), compiled for the host with
-O2 -ffp-contract=off (the kernels' own float operations, bit for bit) and held against the oracle's state arrays.

For every Gaussian the oracle gives a radius > 0 the host build must give the oracle's BITS (compared as uint32): radius, pixel
centre, the three conic floats, view depth, the 3D covariance, the tile-rectangle area (the reference's tiles_touched), rgb and
the clamp bits.  Every other Gaussian must come back culled, with radius 0.  No row is excluded.

Outside this test: the loads, and the raw-mode activations (exp, sigmoid, the quaternion's normalisation) -- the device's expf
is not the host's, so the chain takes activated scales and the quaternion as it uses it, and the callers in preprocess.hip keep
the activations.  tests/test_gpu_raw.py holds those on the GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from luciddreamer_amd import cameras, synthetic
from tests import helpers as hp
from tests import intrinsics_cases as ic
from tests import posed_cases as pc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "luciddreamer_amd", "csrc")

WRAPPER = r"""
#include <stdint.h>
#include "gauss_project.h"
// a view with ViewParams's member names, filled as api.hip fills ViewParams
struct HostView {
    const float *view, *proj, *campos;
    float tan_fovx, tan_fovy, focal_x, focal_y, scale_modifier;
    int W, H, gx, gy, D, M;
};
// What a preprocess kernel does with one Gaussian, minus the record's packing: near plane (auxiliary.h:152-162), 3D
// covariance (given, or from scale and quaternion), the chain, colour (given, or from the SH rows).  Rows of culled Gaussians
// keep their zeros.
extern "C" void gp_run(int P, const float* means, const float* scales, const float* rots, const float* cov_pre, const float* shs,
                       const float* cols_pre, const float* V, const float* Pm, const float* campos, float scale_modifier, int W,
                       int H, float tan_fovx, float tan_fovy, int D, int M, uint8_t* culled, int* radius, float* mean2D,
                       float* conic, float* depth, float* cov3D, uint32_t* area, float* rgb, uint8_t* clamp)
{
    HostView vp;
    vp.view = V; vp.proj = Pm; vp.campos = campos;
    vp.tan_fovx = tan_fovx; vp.tan_fovy = tan_fovy;
    vp.focal_y = H / (2.0f * tan_fovy); vp.focal_x = W / (2.0f * tan_fovx);
    vp.scale_modifier = scale_modifier;
    vp.W = W; vp.H = H; vp.gx = (W + lr::TILE_X - 1) / lr::TILE_X; vp.gy = (H + lr::TILE_Y - 1) / lr::TILE_Y; vp.D = D; vp.M = M;
    for (int i = 0; i < P; i++) {
        culled[i] = 1;
        const float x = means[3 * i], y = means[3 * i + 1], z = means[3 * i + 2];
        const float vz = V[2] * x + V[6] * y + V[10] * z + V[14];
        if (vz <= 0.2f) continue;
        float c3[6];
        if (cov_pre != nullptr) {
            for (int k = 0; k < 6; k++) c3[k] = cov_pre[6 * i + k];
        } else {
            lr::cov3d_scale_rot(scale_modifier * scales[3 * i], scale_modifier * scales[3 * i + 1], scale_modifier * scales[3 * i + 2],
                                rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3], c3);
        }
        lr::GaussProj pj;
        if (!lr::project_chain<false>(vp, x, y, z, c3, pj)) continue;
        culled[i] = 0;
        radius[i] = pj.radius;
        mean2D[2 * i] = pj.pix; mean2D[2 * i + 1] = pj.piy;
        conic[3 * i] = pj.con_a; conic[3 * i + 1] = pj.con_b; conic[3 * i + 2] = pj.con_c;
        depth[i] = pj.vz;
        for (int k = 0; k < 6; k++) cov3D[6 * i + k] = c3[k];
        int minx, miny, maxx, maxy;
        lr::tile_rect(pj.pix, pj.piy, pj.radius, vp.gx, vp.gy, minx, miny, maxx, maxy);
        area[i] = (uint32_t)(maxx - minx) * (uint32_t)(maxy - miny);
        lr::V3 c;
        uint8_t bits = 0;
        if (cols_pre != nullptr) c = { cols_pre[3 * i], cols_pre[3 * i + 1], cols_pre[3 * i + 2] };
        else c = lr::sh_colour(vp, shs, nullptr, (size_t)i, x, y, z, bits);
        rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
        clamp[i] = bits;
    }
}
"""


@pytest.fixture(scope="module")
def gp(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / c++ / clang++) on this machine")
    d = tmp_path_factory.mktemp("gauss_project")
    src, so = d / "gp.cpp", d / "libgp.so"
    src.write_text(WRAPPER)
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.gp_run.restype = None
    L.gp_run.argtypes = [ci] + [vp] * 9 + [cf, ci, ci, cf, cf, ci, ci] + [vp] * 9

    def run(cloud, cam, degree, scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None):
        f = lambda t: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        p = lambda a: None if a is None else a.ctypes.data_as(vp)
        m, cov, cols = f(cloud["means3D"]), f(cov3D_precomp), f(colors_precomp)
        s, q = (None, None) if cov is not None else (f(cloud["scales"]), f(cloud["rotations"]))
        shs = None if cols is not None else f(cloud["shs"])
        V, Pm, cp = f(cam.world_view_transform).reshape(-1), f(cam.full_proj_transform).reshape(-1), f(cam.camera_center)
        P = m.shape[0]
        out = dict(culled=np.zeros(P, np.uint8), radii=np.zeros(P, np.int32), means2D=np.zeros((P, 2), np.float32),
                   conic=np.zeros((P, 3), np.float32), depths=np.zeros(P, np.float32), cov3D=np.zeros((P, 6), np.float32),
                   area=np.zeros(P, np.uint32), rgb=np.zeros((P, 3), np.float32), clamp=np.zeros(P, np.uint8))
        tfx, tfy = hp.tan_fov(cam)
        L.gp_run(P, p(m), p(s), p(q), p(cov), p(shs), p(cols), p(V), p(Pm), p(cp), scale_modifier, cam.image_width,
                 cam.image_height, tfx, tfy, degree, 0 if shs is None else shs.shape[1],
                 *[p(out[k]) for k in ("culled", "radii", "means2D", "conic", "depths", "cov3D", "area", "rgb", "clamp")])
        return out
    return run


BG = torch.zeros(3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _hold(gp, cloud, cam, degree, ref=None, scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None, what=""):
    """The host build of the chain against the oracle's state arrays: bit equality on every row the oracle gives a radius,
    radius 0 / culled on every other.  Returns (oracle radii, host outputs)."""
    if ref is None:
        ref = hp.run_oracle(cloud, cam, degree, BG, colors_precomp=colors_precomp, cov3D_precomp=cov3D_precomp,
                            scale_modifier=scale_modifier)
    st = ref["res"].stage()
    got = gp(cloud, cam, degree, scale_modifier, colors_precomp, cov3D_precomp)
    radii = ref["radii"]
    vis = radii > 0
    assert np.array_equal(got["culled"] == 0, vis), \
        f"{what}: culled differs at rows {np.nonzero((got['culled'] == 0) != vis)[0][:8].tolist()}"
    assert np.array_equal(got["radii"], radii), f"{what}: radii differ at rows {np.nonzero(got['radii'] != radii)[0][:8].tolist()}"
    n = lambda t: t.detach().cpu().numpy()
    pairs = [("means2D", got["means2D"], st["means2D"]), ("conic", got["conic"], st["conic_opacity"][:, :3]),
             ("depths", got["depths"], st["depths"]),
             # the oracle's cov3D array holds what it computed from scale and quaternion; a caller's own covariances are the input
             ("cov3D", got["cov3D"], st["cov3D"] if cov3D_precomp is None else n(cov3D_precomp)),
             ("rgb", got["rgb"], st["rgb"] if colors_precomp is None else n(colors_precomp))]
    for name, a, b in pairs:
        a, b = _bits(a)[vis], _bits(b)[vis]
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs in {bad.size} of {int(vis.sum())} visible rows, first {np.nonzero(vis)[0][bad[:8]].tolist()}"
    assert np.array_equal(got["area"][vis], st["tiles_touched"][vis]), f"{what}: rectangle areas differ"
    assert (got["area"][~vis] == 0).all()
    if colors_precomp is None:
        bits = st["clamped"].astype(np.uint8) @ np.array([1, 2, 4], np.uint8)
        assert np.array_equal(got["clamp"][vis], bits[vis]), f"{what}: clamp bits differ"
    return radii, got


@pytest.mark.parametrize("case", sorted(pc.OP_CASES))
def test_posed_cameras(gp, case):
    """The six camera-frame poses and the four world poses of tests/posed_cases.py, each with its own SH degree."""
    cam, cloud, degree = pc.make(case)
    radii, _ = _hold(gp, cloud, cam, degree, ref=pc.reference(case), what=case)
    assert 0 < (radii > 0).sum()
    if case.startswith("band"):
        assert (radii == 0).sum() > 1000             # behind the camera, across the near plane, off the screen


@pytest.mark.parametrize("case", sorted(ic.CASES))
def test_general_intrinsics(gp, case):
    """The six rows of tests/intrinsics_cases.py: focal_x != focal_y, a shifted principal point, wide and narrow fields of
    view.  Here a focal_x / focal_y mix-up in the chain shows without a GPU."""
    cam, cloud, degree = ic.make(case)
    radii, _ = _hold(gp, cloud, cam, degree, ref=ic.reference(case), what=case)
    assert (radii > 0).sum() >= 0.4 * radii.size


@pytest.fixture(scope="module")
def clouds():
    return {kind: synthetic.make_cloud(20_000, kind, 0) for kind in ("band", "shell")}


@pytest.mark.parametrize("kind", ["band", "shell"])
@pytest.mark.parametrize("res", [(256, 256), (640, 360)])
@pytest.mark.parametrize("mod", [1.0, 0.37])
def test_bench_clouds(gp, clouds, kind, res, mod):
    cam = cameras.rotate360_path(res[0], res[1], n_views=6)[1]
    radii, _ = _hold(gp, clouds[kind], cam, 3, scale_modifier=mod, what=f"{kind} {res} modifier {mod}")
    assert (radii > 0).sum() > 500 and (radii == 0).sum() > 5000


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_degrees(gp, degree):
    """Every degree on the same cloud of 16 coefficients; strong higher bands, so that some channels clamp."""
    cam, cloud = hp.box_setup(3000, 97, 61, seed=3)
    cloud = dict(cloud)
    g = torch.Generator().manual_seed(11)
    cloud["shs"] = cloud["shs"] + 0.8 * torch.randn(cloud["shs"].shape, generator=g) * (torch.arange(16) > 0).float()[None, :, None]
    radii, got = _hold(gp, cloud, cam, degree, what=f"degree {degree}")
    assert (radii > 0).sum() > 1000
    if degree > 0:
        assert (got["clamp"][radii > 0] != 0).sum() > 20


def test_precomputed_covariances_and_colours(gp):
    cam, cloud, cols, cov = pc.precomp_inputs()
    radii, _ = _hold(gp, cloud, cam, 0, ref=pc.precomp_reference(), colors_precomp=cols, cov3D_precomp=cov, what="precomputed")
    assert (radii > 0).sum() > 500


def test_conics_that_are_no_ellipse(gp):
    """The rows of tests/test_gpu_pool_pairs.py::test_conics_that_are_no_ellipse: indefinite 3D covariances of the caller."""
    from tests.test_gpu_pool_pairs import no_ellipse_scene
    cam, cloud = no_ellipse_scene()
    radii, got = _hold(gp, cloud, cam, 3, cov3D_precomp=cloud["cov3D"], what="no ellipse")
    improper = (radii > 0) & ~((got["conic"][:, 0] > 0) & (got["conic"][:, 2] > 0))
    assert improper.sum() > 100


def test_rows_with_a_zero_determinant(gp):
    """det == 0 exactly (forward.cu:219-223): on the axis of an unturned camera with focal / depth = 64 the screen-space
    covariance is 4096 cov3D[0] on its diagonal's first entry, so cov3D[0] = -0.3 / 4096 (exact: a power of two) makes the
    dilated entry 0 and with no off-diagonal term the determinant 0.  The same rows one ulp away are ordinary splats."""
    W = H = 256
    cam = cameras.identity_camera(W, H)
    focal = np.float32(W) / (np.float32(2.0) * np.float32(hp.tan_fov(cam)[0]))
    z = focal / np.float32(64.0)
    assert np.float32(focal / z) == np.float32(64.0)
    P = 64
    rng = np.random.default_rng(17)
    exact = -np.float32(0.3) / np.float32(4096.0)
    cov = np.zeros((P, 6), np.float32)
    cov[:, 0] = exact
    cov[:, 3] = rng.uniform(1e-4, 1e-2, P).astype(np.float32)
    cov[:, 5] = rng.uniform(1e-4, 1e-2, P).astype(np.float32)
    cov[P // 2:, 0] = np.nextafter(exact, np.float32(1.0))        # towards zero: the dilated entry is one ulp above 0
    means = np.zeros((P, 3), np.float32); means[:, 2] = z
    cloud = dict(means3D=torch.from_numpy(means), opacities=torch.full((P, 1), 0.5), shs=torch.rand(P, 16, 3, generator=torch.Generator().manual_seed(1)))
    radii, got = _hold(gp, cloud, cam, 3, cov3D_precomp=torch.from_numpy(cov), what="det == 0")
    assert (radii[:P // 2] == 0).all() and (got["culled"][:P // 2] == 1).all()      # the oracle agrees that these leave at det == 0
    assert (radii[P // 2:] > 0).all()
