"""Inputs of the 3D smoothing filter's tests (tests/test_filter3d_cpu.py, tests/test_gpu_filter3d.py): seeded clouds against
look-around camera paths, and hand-placed rows on both sides of every visibility test.  A case is (xyz [P,3], cams [V,20]) in
float32, cams as luciddreamer_amd.filter3d.pack_cameras lays them out.

No case has a FRAGILE Gaussian-camera pair (tests/filter3d_ref.py: z within 1e-4 relative of 0.2, or a projected coordinate
within 1e-4 relative of its 0.65 bound), where float32 may legitimately decide the test the other way than float64 does: the
builder redraws every point that has one, and tests/test_filter3d_cpu.py asserts that none is left.  The `seen` bytes of a
device run can therefore be compared exactly.
"""
import functools
import math

import numpy as np

from tests import filter3d_ref as R

P_VALUES = (1, 63, 64, 65, 257, 1037)
V_VALUES = (1, 3, 70, 257)                  # 70 and 257 cross the kernel's camera chunk (64) once and four times
W, H = 64, 48


def pack(cams):
    from luciddreamer_amd import filter3d
    return filter3d.pack_cameras(cams, "cpu").numpy()


@functools.lru_cache(maxsize=None)
def path(V):
    from luciddreamer_amd import cameras
    return pack(cameras.lookaround_path(W, H, n_views=V))


def draw(rng, n):
    return np.stack((rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-1, 6, n)), axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def seeded(P, V):
    """x, y in [-3, 3], z in [-1, 6] against lookaround_path(64, 48, V); points with a fragile pair are drawn again."""
    rng = np.random.default_rng(1000 * P + V)
    cams = path(V)
    xyz = draw(rng, P)
    for _ in range(100):
        bad = R.update(xyz, cams, return_fragile=True)[2].any(axis=1)
        if not bad.any():
            return xyz, cams
        xyz[bad] = draw(rng, int(bad.sum()))
    raise AssertionError("could not draw a cloud without fragile pairs")


def identity_cam():
    from luciddreamer_amd import cameras
    return pack([cameras.identity_camera(W, H)])


HAND_ROWS = ("behind", "z=0.19", "z=0.21", "x at 0.64 W", "x at 0.66 W", "y at 0.64 H", "y at 0.66 H", "-x at 0.64 W",
             "x in the margin", "y in the margin", "far off to the side", "on the axis")
HAND_SEEN = (False, False, True, True, False, True, False, True, True, True, False, True)


@functools.lru_cache(maxsize=None)
def hand_placed():
    """The identity camera and one row per side of every test.  Projected coordinates are x / z * fx; the image ends at 0.5 W,
    the margin at 0.65 W."""
    cams = identity_cam()
    fx, fy = float(cams[0, 16]), float(cams[0, 17])
    z = 2.0
    at = lambda frac, size, f: frac * size * z / f
    rows = [(0.0, 0.0, -1.0), (0.0, 0.0, 0.19), (0.0, 0.0, 0.21),
            (at(0.64, W, fx), 0.0, z), (at(0.66, W, fx), 0.0, z), (0.0, at(0.64, H, fy), z), (0.0, at(0.66, H, fy), z),
            (-at(0.64, W, fx), 0.0, z),
            (at(0.58, W, fx), 0.0, z), (0.0, -at(0.58, H, fy), z),
            (100.0, 0.0, 1.0), (0.0, 0.0, 3.0)]
    assert len(rows) == len(HAND_ROWS) == len(HAND_SEEN)
    return np.array(rows, dtype=np.float32), cams


@functools.lru_cache(maxsize=None)
def nothing_seen():
    """A cloud behind the cameras of a three-view path."""
    rng = np.random.default_rng(5)
    xyz = draw(rng, 65)
    xyz[:, 2] = -1.0 - np.abs(xyz[:, 2])
    return xyz, path(3)


@functools.lru_cache(maxsize=None)
def mixed_focal():
    """Two cameras on the z axis looking down +z: A at the origin with a short focal length, B two units further back with a
    focal length four times as long.  For the point (0, 0, 2): z / fx is 2 / fA from A and 4 / (4 fA) = 1 / fA from B, so the
    paper's d = min z / fx = 1 / fA, while min z / max fx (the released code's) = 2 / (4 fA) = 0.5 / fA.  A second point only A
    sees and a third nobody sees ride along."""
    from luciddreamer_amd import cameras
    fov_a = 2 * math.atan(W / (2 * 40.0))                   # fx = 40
    fov_b = 2 * math.atan(W / (2 * 160.0))                  # fx = 160
    back = np.eye(4)
    back[2, 3] = -2.0
    cams = pack([cameras.make_camera(np.eye(4), W, H, fov_a), cameras.make_camera(back, W, H, fov_b)])
    xyz = np.array([(0.0, 0.0, 2.0), (1.2, 0.0, 2.0), (0.0, 50.0, 1.0)], dtype=np.float32)
    return xyz, cams


def all_cases():
    """{name: (xyz, cams)}: what the GPU update test runs and the CPU test checks for fragile pairs."""
    cases = {f"P{P}-V{V}": seeded(P, V) for P in P_VALUES for V in V_VALUES}
    cases["hand-placed"] = hand_placed()
    cases["nothing-seen"] = nothing_seen()
    cases["mixed-focal"] = mixed_focal()
    return cases


CASE_NAMES = tuple([f"P{P}-V{V}" for P in P_VALUES for V in V_VALUES] + ["hand-placed", "nothing-seen", "mixed-focal"])


# ---- inputs of the apply ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def apply_inputs(P):
    """(raw_scale [P,3] in [-12, 2], raw_opacity [P,1] in [-12, 12], filter [P,1] in {0} U [1e-4, 1] log-uniform, upstream
    gradients [P,3], [P,1] ~ N(0, 1)).  With P > 1 every fourth filter is 0, and so is row 0; the single row of P = 1 is a
    filtered one (the pass-through has its rows in every larger case)."""
    rng = np.random.default_rng(7000 + P)
    f = np.exp(rng.uniform(math.log(1e-4), 0.0, (P, 1)))
    off = rng.uniform(size=(P, 1)) < 0.25
    if P > 1:
        f[off] = 0.0
        f[0] = 0.0
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return (f32(rng.uniform(-12, 2, (P, 3))), f32(rng.uniform(-12, 12, (P, 1))), f32(f), f32(rng.normal(size=(P, 3))),
            f32(rng.normal(size=(P, 1))))
