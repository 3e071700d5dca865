"""Seeded cases of the TSDF tests (test helper, not collected): the analytic fields of the extraction tests, the depth frames
of the integration tests and the views of the end-to-end test.  Shared by tests/test_tsdf_cpu.py and tests/test_gpu_tsdf.py;
references are computed once per process (functools.lru_cache) and callers do not modify them."""
import functools
import math

import numpy as np

from tests import posed_cases, tsdf_ref

# ---- analytic fields: volume 20 x 20 x 20, s = 1, trunc = 3, origin 0 ----------------------------------------------------------
FIELD_DIMS, FIELD_S, FIELD_TRUNC = (20, 20, 20), 1.0, 3.0
SPHERE_C, SPHERE_R = np.array([9.3, 9.6, 9.45]), 6.2            # centre off the lattice
TORUS_C, TORUS_R, TORUS_r = np.array([9.4, 9.55, 9.3]), 5.5, 2.4
PLANE_N, PLANE_P = np.array([0.35, 0.25, 0.9]) / np.linalg.norm([0.35, 0.25, 0.9]), np.array([9.5, 9.5, 9.37])
PLANE_X_MAX = 11                                                # weight = 0 for x >= 12
WIDE_DIMS, WIDE_C, WIDE_R = (48, 48, 40), np.array([23.3, 23.6, 19.45]), 15.2     # 7 N / 2048 = 315 scan tiles: more than one
                                                                                # round of the block-sum scan (256 per round)
FIELD_NAMES = ("sphere", "torus", "plane", "sphere_zeroed", "thin", "empty", "wide")


def _grid(dims, s=1.0, origin=(0.0, 0.0, 0.0)):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz) * s + origin[2], np.arange(ny) * s + origin[1], np.arange(nx) * s + origin[0],
                          indexing="ij")
    return x, y, z


def _colors(x, y, z, dims):
    return np.stack([x / dims[0], y / dims[1], 0.25 + 0.5 * z / dims[2]], axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def field(name):
    """RefVolume holding the field `name`: signed distance / trunc clamped to [-1, 1], weight 1 (the plane: 0 for x >= 12)."""
    dims = (65, 5, 3) if name == "thin" else WIDE_DIMS if name == "wide" else FIELD_DIMS
    vol = tsdf_ref.RefVolume((0.0, 0.0, 0.0), FIELD_S, dims, FIELD_TRUNC)
    x, y, z = _grid(dims)
    w = np.ones(x.shape, dtype=np.float32)
    if name in ("sphere", "sphere_zeroed"):
        f = np.sqrt((x - SPHERE_C[0]) ** 2 + (y - SPHERE_C[1]) ** 2 + (z - SPHERE_C[2]) ** 2) - SPHERE_R
        if name == "sphere_zeroed":
            f = np.where(np.abs(f) < 0.25, 0.0, f)              # exact zeros: triangles of zero area
    elif name == "torus":
        rho = np.sqrt((x - TORUS_C[0]) ** 2 + (z - TORUS_C[2]) ** 2) - TORUS_R
        f = np.sqrt(rho ** 2 + (y - TORUS_C[1]) ** 2) - TORUS_r
    elif name == "plane":
        f = PLANE_N[0] * (x - PLANE_P[0]) + PLANE_N[1] * (y - PLANE_P[1]) + PLANE_N[2] * (z - PLANE_P[2])
        w = np.where(x >= PLANE_X_MAX + 1, 0.0, 1.0).astype(np.float32)
    elif name == "thin":
        # partial waves along x, thin y and z: seeded values with exact zeros, weights on both sides of min_weight, one NaN weight
        rng = np.random.default_rng(65)
        f = FIELD_TRUNC * rng.uniform(-1.0, 1.0, x.shape)
        f = np.where(rng.uniform(size=x.shape) < 0.08, 0.0, f)
        w = rng.choice(np.array([0.0, 0.5, 1.0, 2.5], dtype=np.float32), size=x.shape, p=[0.04, 0.04, 0.46, 0.46])
        w[1, 2, 40] = np.nan
    elif name == "wide":
        f = np.sqrt((x - WIDE_C[0]) ** 2 + (y - WIDE_C[1]) ** 2 + (z - WIDE_C[2]) ** 2) - WIDE_R
    elif name == "empty":
        f = np.full(x.shape, FIELD_TRUNC)
        w = np.zeros(x.shape, dtype=np.float32)
    else:
        raise KeyError(name)
    vol.tsdf = np.clip(f / FIELD_TRUNC, -1.0, 1.0).astype(np.float32)
    vol.weight = w
    vol.color = _colors(x, y, z, dims)
    return vol


@functools.lru_cache(maxsize=None)
def field_mesh(name):
    """(vertices, colors, faces) of the restatement for field(name)."""
    return field(name).extract(1.0)


# ---- analytic depth: a sphere in front of a wall -------------------------------------------------------------------------------
def render_depth(K, R, T, H, W, sphere_c, sphere_r, wall_z):
    """Depth (camera z) of a sphere and of the world plane z = wall_z seen from the world-to-camera pose (R, T), float64 per
    pixel centre (pixel index = coordinate), 0 where the ray hits nothing in front of the camera.  float32 [H,W]."""
    K, R, T = np.asarray(K, np.float64), np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1)     # camera frame, z = 1
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        if sphere_r > 0:
            c = R @ np.asarray(sphere_c, np.float64) + T
            a = (ray * ray).sum(-1)
            b = ray @ c
            disc = b * b - a * (c @ c - sphere_r ** 2)
            t = (b - np.sqrt(disc)) / a
            best = np.where((disc >= 0) & (t > 0), np.minimum(best, t), best)
        # world z of the point ray * t: row 2 of R^T (ray t - T)
        n = R[:, 2]
        t = (wall_z + n @ T) / (ray @ n)
        best = np.where(np.isfinite(t) & (t > 0), np.minimum(best, t), best)
    return np.where(np.isfinite(best), best, 0.0).astype(np.float32)


def w2c(pose):
    """(R, T) world to camera of a posed_cases pose (yaw, pitch, roll, translation)."""
    m = np.linalg.inv(posed_cases.c2w_of(pose))
    return np.ascontiguousarray(m[:3, :3]), np.ascontiguousarray(m[:3, 3])


# ---- integration: volume 70 x 18 x 16, frames 24 x 32 ---------------------------------------------------------------------------
INT_DIMS, INT_S, INT_TRUNC, INT_ORIGIN = (70, 18, 16), 0.1, 0.3, (-3.45, -0.83, -0.77)
INT_H, INT_W, INT_F = 24, 32, 11                                 # 11 frames: across the 8-frame launch boundary
INT_K = np.array([[20.0, 0.0, 15.5], [0.0, 20.0, 11.5], [0.0, 0.0, 1.0]])
INT_SPHERE_C, INT_SPHERE_R, INT_WALL_Z = (0.4, 0.05, 0.0), 0.6, 0.55
INT_POSES = [(0.0, 0.0, 0.0, (0.0, 0.0, -3.0)),
             (0.25, 0.0, 0.0, (-0.8, 0.1, -2.9)),
             (-0.3, 0.05, 0.0, (1.0, 0.0, -2.8)),
             (math.pi, 0.0, 0.0, (0.0, 0.0, -3.0)),             # the volume behind the camera
             (0.2, -0.35, 0.6, (-0.6, -1.1, -2.7)),             # pitched and rolled
             (0.0, 0.0, 0.0, (2.2, 0.0, -3.2)),
             (-0.1, 0.1, -0.2, (-2.0, 0.3, -3.0)),
             (0.45, 0.0, 0.0, (-1.6, 0.0, -2.6)),
             (0.0, 0.2, 0.0, (0.3, 0.6, -2.5)),                 # frame 8: the second launch
             (-0.5, 0.0, 0.1, (1.7, -0.2, -2.6)),
             (0.1, -0.1, 0.0, (-0.3, -0.4, -3.4))]


@functools.lru_cache(maxsize=None)
def integrate_inputs():
    """dict(depths [F,H,W], colors [F,H,W,3], pixel_weights [F,H,W] float32, K, Rs [F,3,3], Ts [F,3]): analytic depth with
    seeded pixels of 0, NaN, +inf and negative depth, a weight map with zeros (and one NaN, one negative, one +inf)."""
    assert len(INT_POSES) == INT_F
    rng = np.random.default_rng(11)
    Rs, Ts = zip(*[w2c(p) for p in INT_POSES])
    depths = np.stack([render_depth(INT_K, R, T, INT_H, INT_W, INT_SPHERE_C, INT_SPHERE_R, INT_WALL_Z) for R, T in zip(Rs, Ts)])
    bad = np.array([0.0, np.nan, np.inf, -1.5], dtype=np.float32)
    for f in range(INT_F):
        idx = rng.choice(INT_H * INT_W, size=24, replace=False)
        depths[f].reshape(-1)[idx] = bad[np.arange(24) % 4]
    colors = rng.uniform(0.0, 1.0, (INT_F, INT_H, INT_W, 3)).astype(np.float32)
    pw = rng.uniform(0.25, 2.0, (INT_F, INT_H, INT_W)).astype(np.float32)
    pw[rng.uniform(size=pw.shape) < 0.15] = 0.0
    pw[0, 12, 16], pw[1, 11, 15], pw[2, 12, 14] = np.nan, -1.0, np.inf
    out = dict(depths=depths, colors=colors, pixel_weights=pw, K=INT_K, Rs=np.stack(Rs), Ts=np.stack(Ts))
    for a in out.values():
        a.setflags(write=False)
    return out


# name: (colour, pixel weights, depth_max, max_weight)
INT_VARIANTS = {"plain": (False, False, np.inf, np.inf), "color": (True, False, np.inf, np.inf),
                "weights": (True, True, np.inf, np.inf), "limits": (True, True, 3.3, 2.5)}


def new_int_volume(max_weight=np.inf):
    return tsdf_ref.RefVolume(INT_ORIGIN, INT_S, INT_DIMS, INT_TRUNC, max_weight=max_weight)


@functools.lru_cache(maxsize=None)
def integrate_reference(variant):
    """(RefVolume, touched) of the restatement after the 11 frames."""
    with_color, with_pw, depth_max, max_weight = INT_VARIANTS[variant]
    a = integrate_inputs()
    vol = new_int_volume(max_weight)
    touched = vol.integrate(a["depths"], a["K"], a["Rs"], a["Ts"], colors=a["colors"] if with_color else None,
                            pixel_weights=a["pixel_weights"] if with_pw else None, depth_max=depth_max)
    return vol, touched


# ---- end to end: six views of a sphere into 24^3 --------------------------------------------------------------------------------
E2E_DIMS, E2E_S, E2E_TRUNC, E2E_ORIGIN = (24, 24, 24), 0.1, 0.3, (-1.17, -1.13, -1.21)
E2E_H, E2E_W = 48, 48
E2E_K = np.array([[40.0, 0.0, 23.5], [0.0, 40.0, 23.5], [0.0, 0.0, 1.0]])
E2E_SPHERE_C, E2E_SPHERE_R = (0.03, -0.02, 0.05), 0.7
# the camera on the six axes, looking at the origin (COLMAP axes: z forward)
E2E_POSES = [(0.0, 0.0, 0.0, (0.0, 0.0, -3.0)), (math.pi, 0.0, 0.0, (0.0, 0.0, 3.0)),
             (math.pi / 2, 0.0, 0.0, (-3.0, 0.0, 0.0)), (-math.pi / 2, 0.0, 0.0, (3.0, 0.0, 0.0)),
             (0.0, math.pi / 2, 0.0, (0.0, 3.0, 0.0)), (0.0, -math.pi / 2, 0.0, (0.0, -3.0, 0.0))]


@functools.lru_cache(maxsize=None)
def e2e_inputs():
    Rs, Ts = zip(*[w2c(p) for p in E2E_POSES])
    depths = np.stack([render_depth(E2E_K, R, T, E2E_H, E2E_W, E2E_SPHERE_C, E2E_SPHERE_R, 1e9) for R, T in zip(Rs, Ts)])
    depths[depths > 100.0] = 8.0                                 # a far backdrop: free space is observed as free
    v, u = np.meshgrid(np.arange(E2E_H), np.arange(E2E_W), indexing="ij")
    colors = np.stack([np.stack([u / E2E_W, v / E2E_H, np.full(u.shape, f / 6.0)], -1) for f in range(6)]).astype(np.float32)
    out = dict(depths=depths, colors=colors, K=E2E_K, Rs=np.stack(Rs), Ts=np.stack(Ts))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def e2e_reference():
    """(RefVolume, (vertices, colors, faces)) of the restatement."""
    a = e2e_inputs()
    vol = tsdf_ref.RefVolume(E2E_ORIGIN, E2E_S, E2E_DIMS, E2E_TRUNC)
    vol.integrate(a["depths"], a["K"], a["Rs"], a["Ts"], colors=a["colors"])
    return vol, vol.extract(1.0)
