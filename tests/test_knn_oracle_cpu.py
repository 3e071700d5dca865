"""CPU: the references of the distCUDA2 tests agree with each other on every cloud of tests/knn_cases.py, within the bar the
GPU tests then apply to the HIP kernels (tests/test_gpu_knn.py).

The bar, derived (u = 2^-24): dx = fl(qx - px) is one correctly rounded operation, the same in every float32 implementation.
d = dx*dx + dy*dy + dz*dz is a sum of three non-negative products: at most 3 roundings on the way to it with or without FMA
contraction, no cancellation, so d is within 3u (relative) of the exact value on the same rounded differences.  Order statistics
are monotone: the k-th smallest of the perturbed distances is within 3u of the k-th smallest exact one, whichever neighbour is
picked at a tie.  Two more additions and one division: <= 6u per float32 implementation.  Hence
  float32 against float32 (HIP against oracle_dist2, HIP against the reference's kernels):  |a - b| <= 12u * b
  float32 against the float64 reference, whose differences are exact (+2u for dx*dx):       |a - r| <=  8u * r
with an absolute floor of 4 * FLT_MIN for rows whose squares underflow, +inf equal to +inf, and `==` where the expectation is
exactly 0.0 (a point with three coincident others) or 1.0 (the unit lattice).  The factors are derived, not measured; what this
file measures (printed per case) is how much of them the CPU implementations use.

Cases larger than knn_cases.CPU_MAX_P are generated at that size here: five O(P^2) loops per case."""
import numpy as np
import pytest

from oracle import oracle
from tests import knn_cases as kc


def _points(case):
    return case.make(min(case.P, kc.CPU_MAX_P))


@pytest.mark.parametrize("case", kc.CASES, ids=kc.case_ids())
def test_references_agree_within_the_derived_bar(case):
    pts = _points(case)
    P = pts.shape[0]
    assert pts.dtype == np.float32 and pts.shape == (P, 3) and pts.flags.c_contiguous and np.isfinite(pts).all()
    assert np.array_equal(pts, _points(case)), "generators are seeded"
    full = oracle.dist2(pts)
    f64 = oracle.dist2_f64(pts)
    fma = [oracle.dist2_fma(pts, v) for v in (1, 2)]

    # the subset loops are the full loops, bit for bit (all rows, and a shuffled sample with a repeated row)
    rng = np.random.Generator(np.random.PCG64(P))
    rows = rng.permutation(P)[:max(1, min(P, 257))].astype(np.int32)
    rows = np.concatenate([rows, rows[:1]])
    assert np.array_equal(oracle.dist2_subset(pts, np.arange(P)).view(np.uint32), full.view(np.uint32))
    assert np.array_equal(oracle.dist2_subset(pts, rows).view(np.uint32), full[rows].view(np.uint32))
    assert np.array_equal(oracle.dist2_f64(pts, rows).view(np.uint64), f64[rows].view(np.uint64))
    for v in (1, 2):
        assert np.array_equal(oracle.dist2_fma(pts, v, rows).view(np.uint32), fma[v - 1][rows].view(np.uint32))

    # float32, with and without contraction, within 8u of float64; float32 against float32 within 12u
    worst = {"f32": kc.assert_rows(full, f64, kc.BAR_F64, f"{case.name}: oracle_dist2 vs f64")}
    for v in (1, 2):
        worst[f"fma{v}"] = kc.assert_rows(fma[v - 1], f64, kc.BAR_F64, f"{case.name}: fma variant {v} vs f64")
        worst[f"fma{v}/f32"] = kc.assert_rows(fma[v - 1], full, kc.BAR_F32, f"{case.name}: fma variant {v} vs oracle_dist2")
    print(f"knn-cpu-ratio {case.name} P={P} " + " ".join(f"{k}={w:.3f}u" for k, w in worst.items()))

    # exact expectations
    if P < 4:
        # fewer than 3 other points: FLT_MAX slots.  Two of them overflow the float32 sum (+inf), one gives FLT_MAX / 3
        assert np.all(full >= np.float32(1e38)) and (P == 3 or np.all(np.isposinf(full)))
    zero = kc.zero_rows(pts)
    for name, a in (("f32", full), ("fma1", fma[0]), ("fma2", fma[1]), ("f64", f64)):
        assert np.all(a[zero] == 0.0), (case.name, name)
        if case.exact is not None:
            assert np.all(a == case.exact), (case.name, name)
    if case.exact == 0.0:
        assert zero.all()


def test_the_table_holds_what_the_gpu_tests_rely_on():
    names = set(kc.case_ids())
    assert len(names) == len(kc.CASES)
    for need in ("box", "band", "shell", "surface", "duplicates", "all_identical", "line_zero", "line_const", "plane_zero",
                 "plane_const", "offset_positive", "offset_negative", "clusters", "lattice", "lattice_tenth"):
        assert need in names
    for P in kc.SIZES:
        assert f"box_{P}" in names and f"surface_{P}" in names
    assert max(c.P for c in kc.CASES) <= 100_000 and all(c.P <= 50_000 for c in kc.CASES if c.name.startswith("offset"))

    d = kc.duplicates(30_000)
    _, cnt = np.unique(d, axis=0, return_counts=True)
    assert (cnt == 2).sum() == 375 and (cnt == 4).sum() == 187 and (cnt == 1001).sum() == 1 and cnt.max() == 1001
    assert 0.045 < (cnt[cnt > 1].sum() - 1001) / 30_000 < 0.055
    assert kc.zero_rows(d).sum() == 4 * 187 + 1001

    s = kc.surface(196_608, 1)                                      # the full 256 x 256 x 3 grid, in view-then-pixel order
    r = np.linalg.norm(s.astype(np.float64), axis=1)
    assert 1.0 < r.min() < 2.5 and 4.5 < r.max() < 6.0
    jump = np.abs(np.diff(r[:65_536].reshape(256, 256), axis=1))
    assert (jump > 0.5).sum() >= 100, "depth discontinuities inside a view"
    assert kc.surface(5, 3).shape == (5, 3)

    c = kc.clusters(100_000)
    assert (np.abs(c).max(axis=1) > 20.0).sum() >= 900, "outliers far outside the 10-unit box"
    o = kc.offset(1000, (100.0, 100.0, 100.0))
    assert o.min() > 99.0 and o.max() < 101.0
    assert np.all(kc.line(100, 0.0)[:, 1:] == 0.0) and np.all(kc.plane(100, -0.6)[:, 2] == np.float32(-0.6))
    lat = kc.lattice(27_000)
    assert lat.shape == (27_000, 3) and np.array_equal(np.unique(lat), np.arange(30, dtype=np.float32))


def test_row_bar_rules():
    inf = np.inf
    r = kc.row_ratio(np.array([1.0, inf, inf, 1.0, 0.0, np.nan, 0.0, 1e-39], np.float32),
                     np.array([1.0, inf, 1.0, inf, 0.0, 1.0, 1e-30, 0.0], np.float64))
    assert r[0] == 0 and r[1] == 0 and r[2] == inf and r[3] == inf and r[4] == 0 and r[5] == inf and r[6] > 1e6 and r[7] == 0
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    assert kc.row_ratio(np.array([up]), np.array([1.0]))[0] == 2.0                     # one ulp above 1.0 is 2u
    with pytest.raises(AssertionError, match="beyond the bar"):
        kc.assert_rows(np.array([1.0 + 13 * kc.U]), np.array([1.0]), kc.BAR_F32, "x")
    assert kc.assert_rows(np.array([1.0 + 12 * kc.U]), np.array([1.0]), kc.BAR_F32, "x") == 12.0


def test_old_absolute_bar_is_blind_on_clusters():
    """Why the bar is per row: on `clusters` a row that is wrong by 100 % passes max|a - b| <= 1e-6 * b.max()."""
    pts = kc.clusters(kc.CPU_MAX_P)
    ref = oracle.dist2(pts)
    bad = ref.copy()
    small = ref < 1e-6
    assert small.sum() > 0.9 * ref.size
    bad[small] *= 2.0
    assert np.abs(bad - ref).max() <= 1e-6 * ref.max()
    with pytest.raises(AssertionError):
        kc.assert_rows(bad, ref, kc.BAR_F32, "clusters")
