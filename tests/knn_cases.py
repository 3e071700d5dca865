"""Seeded point clouds of the distCUDA2 tests (test helper, not collected), shared by tests/test_knn_oracle_cpu.py -- which checks
on the CPU that the references agree with each other on them within the derived tolerance -- and tests/test_gpu_knn.py /
tests/test_gpu_reference_on_device.py, which feed the same list to the HIP kernels.  Every generator returns float32 (P, 3).

The tolerance (see tests/test_knn_oracle_cpu.py for the derivation) lives here too, so that both sides apply the same rule:
per row |a - ref| <= factor * u * ref with u = 2^-24, an absolute floor of 4 * FLT_MIN, +inf equal to +inf."""
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
FLOOR = 4.0 * FLT_MIN
BAR_F32 = 12.0           # float32 implementation against float32 implementation (6u each)
BAR_F64 = 8.0            # float32 implementation against the float64 reference (6u + 2u for the rounded differences)

SIZES = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 65_537)
CPU_MAX_P = 20_000       # the CPU test runs five O(P^2) loops per case: larger cases are generated at this size there


# ---------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def synthetic_cloud(kind, P, seed):
    """box / band / shell of luciddreamer_amd.synthetic.make_cloud (shell: LucidDreamer's scene statistics)."""
    from luciddreamer_amd import synthetic
    return np.ascontiguousarray(synthetic.make_cloud(P, kind, seed, sh_coeffs=1)["means3D"].numpy(), dtype=np.float32)


def _radius(az, el):
    """The scene seen from the origin: a smooth radial surface, and three foreground discs (in angle) at 0.45 of its depth --
    the depth discontinuities.  Range about 1.2 .. 5.5."""
    r = 4.0 + np.sin(3.0 * az) * np.cos(2.0 * el) + 0.3 * np.sin(11.0 * az + 5.0 * el)
    for a0, e0, rad in ((-0.25, 0.05, 0.12), (0.2, -0.1, 0.08), (0.45, 0.12, 0.1)):
        r = np.where((az - a0) ** 2 + (el - e0) ** 2 < rad * rad, 0.45 * r, r)
    return r


def surface(P, seed=0, n_views=3):
    """What create_from_pcd receives: a W x H pixel grid unprojected through a pinhole camera (focal 1.14 W: the reference's
    512-pixel views have about that field) with a depth map that is smooth apart from a few discontinuities, for n_views views
    that turn about the origin by 20 degrees each, concatenated in view-then-pixel order.  Neighbouring views overlap by about
    half and sample the same surface on different grids: near-coincident points; the foreground discs are sampled denser than
    what is behind them: density jumps.  256 x 256 per view up to 196 608 points (fewer: an ordered random subset), a larger grid
    beyond."""
    side = max(256, int(math.ceil(math.sqrt(P / float(n_views)))))
    rng = _rng(1000 + seed)
    f = 1.14 * side
    x, y = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64), indexing="xy")
    cx = (side - 1) * 0.5
    ray = np.stack([(x - cx) / f, (y - cx) / f, np.ones_like(x)], axis=-1).reshape(-1, 3)
    ray /= np.linalg.norm(ray, axis=1, keepdims=True)
    parts = []
    for v in range(n_views):
        yaw = math.radians(20.0) * (v - (n_views - 1) * 0.5) + 1e-3 * rng.standard_normal()
        c, s = math.cos(yaw), math.sin(yaw)
        d = ray @ np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
        az, el = np.arctan2(d[:, 0], d[:, 2]), np.arcsin(np.clip(d[:, 1], -1.0, 1.0))
        parts.append((d * _radius(az, el)[:, None]).astype(np.float32))
    pts = np.concatenate(parts)
    if P < pts.shape[0]:
        pts = pts[np.sort(rng.choice(pts.shape[0], size=P, replace=False))]
    assert pts.shape[0] == P
    return np.ascontiguousarray(pts)


def duplicates(P, seed=0):
    """Uniform cloud where 5 % of the points are exact copies in groups of 2 and of 4, plus one blob of 1 000 identical points
    (more than a box of 256 holds: at least 4 boxes with a zero-extent AABB).  Shuffled."""
    rng = _rng(2000 + seed)
    blob = min(1000, P // 4)
    n4 = (P // 40) // 4            # 2.5 % of the rows in groups of 4
    n2 = (P // 40) // 2            # 2.5 % in groups of 2
    base = P - blob - 3 * n4 - n2
    pts = rng.uniform(-1.0, 1.0, size=(base, 3)) * (2.0, 1.2, 1.5) + (0.0, 0.0, 4.0)
    src = rng.permutation(base)
    g4, g2 = src[:n4], src[n4:n4 + n2]
    out = np.concatenate([pts, np.repeat(pts[g4], 3, axis=0), pts[g2], np.repeat(pts[src[-1:]], blob, axis=0)])
    assert out.shape[0] == P
    return np.ascontiguousarray(out[rng.permutation(P)].astype(np.float32))


def all_identical(P, seed=0):
    return np.ascontiguousarray(np.tile(np.array([[0.3, -1.2, 2.5]], dtype=np.float32), (P, 1)))


def line(P, const, seed=0):
    """Points on a line along x: y and z constant (0.0: the scene box has zero extent on those axes; otherwise the origin seed
    gives them an extent and every point sits at its far end)."""
    pts = np.full((P, 3), const, dtype=np.float64)
    pts[:, 0] = _rng(3000 + seed).uniform(-2.0, 3.0, size=P)
    return np.ascontiguousarray(pts.astype(np.float32))


def plane(P, const, seed=0):
    pts = np.full((P, 3), const, dtype=np.float64)
    pts[:, :2] = _rng(3500 + seed).uniform(-2.0, 3.0, size=(P, 2))
    return np.ascontiguousarray(pts.astype(np.float32))


def offset(P, centre, seed=0):
    """Unit-extent uniform cloud far from the origin: the origin-seeded scene box is 100 times the cloud, the Morton codes fall
    into a few cells, box pruning does nothing (O(P^2) on the device as in the reference): keep P small."""
    return np.ascontiguousarray((_rng(4000 + seed).uniform(-0.5, 0.5, size=(P, 3)) + centre).astype(np.float32))


def clusters(P, seed=0):
    """20 clusters of sigma 1e-4 in a 10-unit box and 1 % outliers on the scale of 1e3: rows whose value is 1e-8 next to rows
    whose value is 1e5 -- an absolute bar set by the largest row sees nothing of the former."""
    rng = _rng(5000 + seed)
    n_out = P // 100
    centres = rng.uniform(0.0, 10.0, size=(20, 3))
    which = rng.integers(0, 20, size=P - n_out)
    pts = centres[which] + 1e-4 * rng.standard_normal(size=(P - n_out, 3))
    out = np.concatenate([pts, rng.uniform(-1e3, 1e3, size=(n_out, 3))])
    return np.ascontiguousarray(out[rng.permutation(P)].astype(np.float32))


def lattice(P, scale=1.0, seed=0):
    """Integer grid n x n x n (n = cube root of P, at least 2), shuffled.  Every point has at least three neighbours at distance
    1 and none closer: at scale 1 the result is exactly 1.0f everywhere, whichever of the tied neighbours is picked."""
    n = max(2, int(round(P ** (1.0 / 3.0))))
    g = np.arange(n, dtype=np.float64)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * scale
    return np.ascontiguousarray(pts[_rng(6000 + seed).permutation(pts.shape[0])].astype(np.float32))


# name, make(P) -> points, P of the GPU comparison, value every row must equal exactly (or None)
Case = namedtuple("Case", "name make P exact")

CASES = [
    Case("box", lambda P: synthetic_cloud("box", P, 4), 30_000, None),
    Case("band", lambda P: synthetic_cloud("band", P, 5), 30_000, None),
    Case("shell", lambda P: synthetic_cloud("shell", P, 6), 30_000, None),
    Case("surface", lambda P: surface(P, 0), 100_000, None),
    Case("duplicates", lambda P: duplicates(P, 0), 30_000, None),
    Case("all_identical", all_identical, 1_000, 0.0),
    Case("all_identical_4", all_identical, 4, 0.0),
    Case("line_zero", lambda P: line(P, 0.0), 30_000, None),
    Case("line_const", lambda P: line(P, 0.37), 30_000, None),
    Case("plane_zero", lambda P: plane(P, 0.0), 30_000, None),
    Case("plane_const", lambda P: plane(P, -0.6), 30_000, None),
    Case("offset_positive", lambda P: offset(P, (100.0, 100.0, 100.0)), 20_000, None),
    Case("offset_negative", lambda P: offset(P, (-100.0, -100.0, -100.0), 1), 20_000, None),
    Case("clusters", lambda P: clusters(P, 0), 100_000, None),
    Case("lattice", lambda P: lattice(P), 27_000, 1.0),
    Case("lattice_2", lambda P: lattice(P), 8, 1.0),
    Case("lattice_tenth", lambda P: lattice(P, 0.1), 27_000, None),
]
CASES += [Case(f"box_{P}", lambda P, _s=P: synthetic_cloud("box", P, 100 + _s % 97), P, None) for P in SIZES]
CASES += [Case(f"surface_{P}", lambda P, _s=P: surface(P, 100 + _s % 97), P, None) for P in SIZES]
BY_NAME = {c.name: c for c in CASES}


def case_ids():
    return [c.name for c in CASES]


def zero_rows(pts):
    """Rows whose point occurs at least 4 times: three other points at distance exactly 0, so the result is exactly 0.0."""
    _, inv, cnt = np.unique(np.ascontiguousarray(pts, dtype=np.float32), axis=0, return_inverse=True, return_counts=True)
    return cnt[inv.reshape(-1)] >= 4


# ---------------------------------------------------------------------------------------------------------------------------
# the per-row bar
# ---------------------------------------------------------------------------------------------------------------------------
def row_ratio(a, ref):
    """|a - ref| / (u * ref) per row, in float64.  Rows within the absolute floor count as 0; rows where both are +inf count as 0;
    a row where only one is infinite, or either is NaN, counts as +inf."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    out = np.full(a.shape, np.inf)
    fin = np.isfinite(a) & np.isfinite(ref)
    err = np.abs(np.where(fin, a, 0.0) - np.where(fin, ref, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err <= FLOOR, 0.0, err / (U * np.abs(np.where(fin, ref, 1.0))))
    out[fin] = r[fin]
    out[np.isposinf(a) & np.isposinf(ref)] = 0.0
    return out


def assert_rows(a, ref, factor, label):
    """Every row within factor * u of ref (no exempted rows); returns the worst ratio for the record."""
    r = row_ratio(a, ref)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= factor:
        i = int(np.argmax(r))
        raise AssertionError(f"{label}: row {i}: got {np.asarray(a)[i]!r}, reference {np.asarray(ref)[i]!r}: {r[i]:.3g} u "
                             f"(bar {factor} u); {int((r > factor).sum())} of {r.size} rows beyond the bar")
    return worst
