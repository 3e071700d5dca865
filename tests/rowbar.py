"""The per-row gradient bar (test helper, not collected).

helpers.compare_grads and helpers.compare_grads_by_row scale their tolerance by the largest entry of the WHOLE tensor, so a
row whose own gradient is small next to that maximum -- an occluded Gaussian, a term that is never the large one -- is barely
checked: it could be zero or garbage.  row_bar holds every row of a [P, ...] gradient to its OWN scale:

    row_max = max|ref64[row]|        err = max|got[row] - ref64[row]|
    e32[row] = the largest distance of any calibrator from ref64 on that row
    a row passes if   err <= max(GRAD_RTOL * row_max, E32_MARGIN * e32[row])

ref64 is a float64 evaluation of the gradient, a calibrator a float32 CPU evaluation of the same gradient (the C oracle, the
torch restatement run in float32): what float32 costs on that very row, cancellation included.  Neither number is new:
GRAD_RTOL is helpers.GRAD_RTOL applied to the row instead of the tensor, and E32_MARGIN = 4 over a float32 restatement's own
distance is the margin of tests/test_gpu_mcmc.py (the kernel sums a row's pixels in another order than either restatement).

  * a row with row_max == 0 must be exactly zero;
  * a row that is all zero in `got` but not in ref64 fails whatever its size;
  * a row that fails may be excused only if it is listed in `fragile_rows` -- the Gaussians that touch a pixel the C oracle flags
    as sitting on a discrete threshold (helpers.touches_fragile, the rule of helpers.compare_grads_by_row) -- and at most
    MAX_EXCUSED rows per tensor and case are."""
import numpy as np

from tests import helpers as hp

E32_MARGIN = 4.0
MAX_EXCUSED = 2


def fragile_rows_of(ref_c):
    """The rows that may be excused: indices of the visible Gaussians of a C-oracle result (helpers.run_oracle's dict) that touch
    a threshold-fragile pixel."""
    st = ref_c["res"].stage()
    if not (st["fragile"] != 0).any():
        return frozenset()
    return frozenset(int(i) for i in np.nonzero(ref_c["radii"] > 0)[0] if hp.touches_fragile(st, i))


def judge(got, ref64, calibrators, fragile_rows=None):
    """One tensor, reshaped to [P, -1].  Returns the report without asserting: dict(worst = largest err / row_max over the rows with
    a non-zero reference, above_floor = rows with err > GRAD_RTOL * row_max (they pass by the calibrator's arm, are excused, or
    fail), excused = [rows], failed = [(row, reason)], rows = P)."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    P = ref64.shape[0]
    b = ref64.reshape(P, -1)
    a = np.asarray(got, dtype=np.float64).reshape(P, -1)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert len(calibrators) >= 1
    e32 = np.zeros(P)
    for c in calibrators:
        c = np.asarray(c, dtype=np.float64).reshape(P, -1)
        assert c.shape == b.shape, (c.shape, b.shape)
        e32 = np.maximum(e32, np.abs(c - b).max(axis=1))
    row_max = np.abs(b).max(axis=1)
    with np.errstate(invalid="ignore"):
        err = np.abs(a - b).max(axis=1)
        floor = hp.GRAD_RTOL * row_max
        live = row_max > 0
        ok = err <= np.maximum(floor, E32_MARGIN * e32)              # NaN in `got`: False
        got_zero = ~np.any(a != 0, axis=1)
        ok = np.where(live, ok & ~got_zero, got_zero)
        above = live & ~(err <= floor)
        rel = np.where(live, err / np.where(live, row_max, 1.0), 0.0)
    fragile = frozenset() if fragile_rows is None else frozenset(int(i) for i in fragile_rows)
    excused, failed = [], []
    for i in np.nonzero(~ok)[0]:
        i = int(i)
        if not live[i]:
            reason = f"reference row is zero, got max {np.abs(a[i]).max():.3e}"
        elif got_zero[i]:
            reason = f"row is all zero, reference max {row_max[i]:.3e}"
        else:
            reason = f"err {err[i]:.3e} = {rel[i]:.2e} of the row max {row_max[i]:.3e}, float32 restatements within {e32[i]:.3e}"
        if i in fragile and len(excused) < MAX_EXCUSED:
            excused.append(i)
        else:
            failed.append((i, reason + (" (touches a fragile pixel, but the excuses are used up)" if i in fragile else "")))
    worst = float(np.nanmax(rel)) if P else 0.0
    if np.isnan(rel).any():
        worst = float("nan")
    return dict(worst=worst, above_floor=int(above.sum()), excused=excused, failed=failed, rows=P)


def row_bar(got, ref64, calibrators, fragile_rows=None, what=""):
    """judge(), asserted: no failed row.  Returns the report."""
    rep = judge(got, ref64, calibrators, fragile_rows)
    assert not rep["failed"], f"{what}: {len(rep['failed'])} of {rep['rows']} rows outside the per-row bar: {rep['failed'][:5]}"
    return rep


def check_all(got, ref64, calibrators, names, fragile_rows=None, what=""):
    """row_bar for every tensor in `names` (dicts of arrays; calibrators: a list of such dicts).  Prints one line of figures per
    call and returns {name: report}."""
    reports = {k: judge(got[k], ref64[k], [c[k] for c in calibrators], fragile_rows) for k in names}
    print(f"[rowbar] {what}: " + ", ".join(
        f"{k} {r['worst']:.1e}/{r['above_floor']}/{len(r['excused'])}" for k, r in reports.items()) +
        "  (worst err/row_max / rows above the floor / rows excused)")
    for k, r in reports.items():
        assert not r["failed"], f"{what}, {k}: {len(r['failed'])} of {r['rows']} rows outside the per-row bar: {r['failed'][:5]}"
    return reports
