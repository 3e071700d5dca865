"""CPU: the 3D smoothing filter without a device.  The float64 reference (tests/filter3d_ref.py) against closed forms, the
backward table against float64 autograd and central differences, the float32 restatement against the reference, the absence
of fragile pairs in every GPU case, the C entries' argument checks (which sit in front of their first HIP call), the header
and the exports, and the Python module's refusals."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import filter3d_cases as C
from tests import filter3d_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lr_filter3d_workspace_bytes", "lr_filter3d_update", "lr_filter3d_apply_forward", "lr_filter3d_apply_backward")


# ---- the reference itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", [0.21, 1.0, 3.0, 57.0])
def test_on_axis_point_under_the_identity_camera(z):
    cams = C.identity_cam()
    filt, seen = R.update(np.array([[0.0, 0.0, z]], dtype=np.float32), cams)
    assert seen[0]
    assert abs(filt[0] - math.sqrt(0.2) * float(np.float32(z)) / float(cams[0, 16])) <= 1e-15 * filt[0] + 1e-18
    assert abs(float(cams[0, 16]) - C.W / (2 * math.tan(0.8279103882874479 / 2))) < 1e-5


def test_hand_placed_rows_fall_on_the_intended_side():
    xyz, cams = C.hand_placed()
    for T in (np.float64, np.float32):
        filt, seen = R.update(xyz, cams, dtype=T)
        assert tuple(bool(s) for s in seen) == C.HAND_SEEN, T
        # unseen rows carry the widest filter in use: the on-axis point at depth 3
        assert np.all(filt[~seen] == filt[seen].max()) and filt[seen].max() == filt[-1]


def test_nothing_seen_and_no_cameras_give_zero():
    xyz, cams = C.nothing_seen()
    for T in (np.float64, np.float32):
        filt, seen = R.update(xyz, cams, dtype=T)
        assert not seen.any() and not filt.any()
        filt, seen = R.update(xyz, cams[:0], dtype=T)
        assert not seen.any() and not filt.any() and filt.shape == (65,)


def test_mixed_focal_lengths_pin_the_papers_definition():
    """min over cameras of z / fx, NOT min z / max fx (Mip-Splatting's released code): the nearer camera has the shorter focal
    length, so the two differ by a factor of two on the first point."""
    xyz, cams = C.mixed_focal()
    fa, fb = float(cams[0, 16]), float(cams[1, 16])
    assert abs(fa - 40) < 1e-4 and abs(fb - 160) < 1e-3
    filt, seen = R.update(xyz, cams)
    assert list(seen) == [True, True, False]
    sv = math.sqrt(0.2)
    assert abs(filt[0] - sv * 4.0 / fb) < 1e-12                  # camera B: farther, but sampling more finely
    assert abs(filt[0] - sv * 2.0 / fb) > 0.4 * filt[0]          # the released code's value is half of it
    assert abs(filt[1] - sv * 2.0 / fa) < 1e-12 and filt[2] == filt[1]


@pytest.mark.parametrize("activated", [False, True])
def test_zero_filter_is_the_identity(activated):
    r, q, f, _, _ = C.apply_inputs(65)
    zero = np.zeros_like(f)
    s64, o64 = R.apply64(r, q, zero, activated)
    s32, o32 = R.apply32(r, q, zero, activated)
    if activated:
        assert np.allclose(s64, np.exp(r.astype(np.float64)), rtol=1e-15) and np.allclose(o64, R.sigmoid(q.astype(np.float64))[:, 0], rtol=1e-14)
    else:
        assert np.array_equal(s64, r.astype(np.float64)) and np.array_equal(o64, q.astype(np.float64)[:, 0])
        assert np.array_equal(s32.view(np.uint32), r.view(np.uint32)) and np.array_equal(o32.view(np.uint32), q[:, 0].view(np.uint32))


def test_filtered_variance_is_the_sum_and_the_opacity_scales_with_the_volume():
    r, q, f, _, _ = C.apply_inputs(257)
    s, o = R.apply64(r, q, f, True)
    s0 = np.exp(r.astype(np.float64))
    assert np.allclose(s ** 2, s0 ** 2 + f.astype(np.float64) ** 2, rtol=1e-13)
    assert np.allclose(o, R.sigmoid(q.astype(np.float64))[:, 0] * np.sqrt(np.prod(s0 ** 2, axis=1) / np.prod(s ** 2, axis=1)), rtol=1e-12)
    ls, lo = R.apply64(r, q, f, False)
    assert np.allclose(np.exp(ls), s, rtol=1e-13)
    assert np.allclose(1.0 / (1.0 + np.exp(-lo)), o, rtol=1e-11, atol=0)


def test_extreme_row_is_finite_in_the_reference_and_the_restatement():
    r, q, f = np.full((1, 3), -40, np.float32), np.full((1, 1), 3, np.float32), np.ones((1, 1), np.float32)
    g, go = np.ones((1, 3), np.float32), np.ones((1, 1), np.float32)
    for act in (False, True):
        for out in (R.apply64(r, q, f, act), R.apply32(r, q, f, act), R.backward64(r, q, f, g, go, act), R.backward32(r, q, f, g, go, act)):
            assert all(np.isfinite(a).all() for a in out), act
    assert np.allclose(R.apply32(r, q, f, True)[0], 1.0, rtol=1e-6) and abs(R.apply32(r, q, f, False)[1][0] + 120 - math.log(1 / (1 + math.exp(-3.0)))) < 1e-4


def _torch_apply(r, q, f, activated):
    """The composition a user writes today, in float64 torch: the autograd reference of the backward table."""
    s2 = torch.exp(2 * r) + f ** 2
    c = torch.sqrt(torch.prod(torch.exp(2 * r), dim=1, keepdim=True) / torch.prod(s2, dim=1, keepdim=True))
    o = torch.sigmoid(q) * c
    if activated:
        return torch.sqrt(s2), o
    return 0.5 * torch.log(s2), torch.log(o) - torch.log1p(-o)


@pytest.mark.parametrize("activated", [False, True])
def test_backward_table_against_float64_autograd(activated):
    """Rows whose scale the composition itself can carry (exp(2 r) and the product of three of them stay normal, 1 - o does
    not cancel): r in [-6, 2], q in [-8, 8].  Largest relative difference 2e-10 in the issue; 1e-8 asked here."""
    rng = np.random.default_rng(3)
    P = 200
    r, q = rng.uniform(-6, 2, (P, 3)), rng.uniform(-8, 8, (P, 1))
    f = np.exp(rng.uniform(math.log(1e-4), 0, (P, 1)))
    f[::5] = 0.0
    g, go = rng.normal(size=(P, 3)), rng.normal(size=(P, 1))
    rt, qt = torch.from_numpy(r).requires_grad_(True), torch.from_numpy(q).requires_grad_(True)
    s, o = _torch_apply(rt, qt, torch.from_numpy(f), activated)
    torch.autograd.backward([s, o], [torch.from_numpy(g), torch.from_numpy(go)])
    dr, dq = R.backward64(r, q, f, g, go, activated)
    for got, want in ((dr, rt.grad.numpy()), (dq, qt.grad.numpy()[:, 0])):
        assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max()
    # the float32 restatement computes the same thing
    r32, q32, f32, g32, go32 = (a.astype(np.float32) for a in (r, q, f, g, go))
    dr32, dq32 = R.backward32(r32, q32, f32, g32, go32, activated)
    dr64, dq64 = R.backward64(r32, q32, f32, g32, go32, activated)
    assert np.abs(dr32 - dr64).max() <= 1e-4 * np.abs(dr64).max() and np.abs(dq32 - dq64).max() <= 1e-4 * np.abs(dq64).max()


@pytest.mark.parametrize("activated", [False, True])
def test_backward_table_against_central_differences(activated):
    rng = np.random.default_rng(4)
    P = 50
    r, q = rng.uniform(-6, 2, (P, 3)), rng.uniform(-8, 8, (P, 1))
    f = np.exp(rng.uniform(math.log(1e-3), 0, (P, 1)))
    g, go = rng.normal(size=(P, 3)), rng.normal(size=(P, 1))

    def loss(r_, q_):
        s, o = R.apply64(r_, q_, f, activated)
        return (s * g).sum(axis=1) + o * go[:, 0]                    # per row: rows are independent
    dr, dq = R.backward64(r, q, f, g, go, activated)
    eps = 1e-6
    for j in range(3):
        e = np.zeros((1, 3))
        e[0, j] = eps
        num = (loss(r + e, q) - loss(r - e, q)) / (2 * eps)
        assert np.abs(num - dr[:, j]).max() <= 1e-6 * max(1.0, np.abs(dr[:, j]).max())
    num = (loss(r, q + eps) - loss(r, q - eps)) / (2 * eps)
    assert np.abs(num - dq).max() <= 1e-6 * max(1.0, np.abs(dq).max())


@pytest.mark.parametrize("P", [1, 63, 1037])
def test_float32_restatement_is_close_to_the_reference(P):
    """The issue's figure for the stored logit in this form: 2.7e-6 absolute over these ranges."""
    r, q, f, _, _ = C.apply_inputs(P)
    for act in (False, True):
        s64, o64 = R.apply64(r, q, f, act)
        s32, o32 = R.apply32(r, q, f, act)
        assert s32.dtype == np.float32 and o32.dtype == np.float32
        assert np.abs(s32 - s64).max() <= 2e-6 * max(1.0, np.abs(s64).max())
        assert np.abs(o32 - o64).max() <= 1e-5


# ---- the GPU cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_gpu_cases_have_no_fragile_pair(name):
    """The allowed number of fragile pairs in a case the device's `seen` bytes are compared on is zero; and float32 then decides
    every visibility test as float64 does."""
    xyz, cams = C.all_cases()[name]
    f64, seen64, fragile = R.update(xyz, cams, return_fragile=True)
    assert int(fragile.sum()) == 0
    f32, seen32 = R.update(xyz, cams, dtype=np.float32)
    assert np.array_equal(seen64, seen32)
    assert np.abs(f32 - f64).max() <= 1e-6 * max(f64.max(), 1e-30)


def test_case_names_cover_the_sizes():
    assert set(C.all_cases()) == set(C.CASE_NAMES)
    assert C.seeded(1037, 257)[0].shape == (1037, 3) and C.seeded(1037, 257)[1].shape == (257, 20)
    seen = R.update(*C.seeded(1037, 70))[1]
    assert 100 < seen.sum() < 1037                                  # both kinds of rows


# ---- the C ABI on a machine without a device -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


def test_header_library_and_binding_agree(L):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lucid_raster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lr_filter3d_[a-z0-9_]+)\s*\(", text))
    assert declared == set(SYMBOLS)
    from luciddreamer_amd import _lib
    assert set(n for n in _lib.EXPORTS if "filter3d" in n) == set(SYMBOLS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes is not None, name


def test_workspace_size_is_a_pure_host_function(L):
    w = L.lr_filter3d_workspace_bytes
    assert w(0) > 0 and w(1) % 256 == 0 and w(1_000_000) >= 4 * ((1_000_000 + 255) // 256)
    assert w(1000) <= w(100_000) < w(10_000_000)


_BUF = (ctypes.c_float * 72)()
PTR = (ctypes.addressof(_BUF) + 15) & ~15               # non-NULL, never dereferenced by the checks


def test_update_rejects_without_a_device(L):
    from luciddreamer_amd import _lib
    bad = _lib.LR_ERR_INVALID_ARG
    assert L.lr_filter3d_update(0, 0, None, None, 0.2, None, None, None, None) == 0
    assert L.lr_filter3d_update(0, 5, None, None, 0.2, None, None, None, None) == 0
    assert L.lr_filter3d_update(-1, 1, PTR, PTR, 0.2, PTR, None, PTR, None) == bad and b"P and V" in L.lr_last_error()
    assert L.lr_filter3d_update(4, -1, PTR, PTR, 0.2, PTR, None, PTR, None) == bad and b"P and V" in L.lr_last_error()
    for v in (-0.1, float("nan"), float("inf")):
        assert L.lr_filter3d_update(4, 1, PTR, PTR, v, PTR, None, PTR, None) == bad and b"variance" in L.lr_last_error()
    for args in ((None, PTR, PTR, PTR), (PTR, None, PTR, PTR), (PTR, PTR, None, PTR), (PTR, PTR, PTR, None)):
        m, c, f, w = args
        assert L.lr_filter3d_update(4, 1, m, c, 0.2, f, None, w, None) == bad and b"required" in L.lr_last_error()


def test_apply_rejects_without_a_device(L):
    from luciddreamer_amd import _lib
    bad = _lib.LR_ERR_INVALID_ARG
    for act in (0, 1):
        assert L.lr_filter3d_apply_forward(0, None, None, None, act, None, None, None) == 0
        assert L.lr_filter3d_apply_backward(0, None, None, None, act, None, None, None, None, None) == 0
        assert L.lr_filter3d_apply_forward(-1, PTR, PTR, PTR, act, PTR, PTR, None) == bad
        assert L.lr_filter3d_apply_backward(-1, PTR, PTR, PTR, act, PTR, PTR, PTR, PTR, None) == bad
        for k in range(5):
            a = [PTR] * 5
            a[k] = None
            assert L.lr_filter3d_apply_forward(4, a[0], a[1], a[2], act, a[3], a[4], None) == bad and b"required" in L.lr_last_error()
            assert L.lr_filter3d_apply_backward(4, a[0], a[1], a[2], act, PTR, PTR, a[3], a[4], None) == bad
            assert b"required" in L.lr_last_error()


# ---- the module ------------------------------------------------------------------------------------------------------
def test_package_exports_the_module_lazily():
    import luciddreamer_amd
    assert callable(luciddreamer_amd.filter3d.filtered) and callable(luciddreamer_amd.filter3d.compute_filter_3d)


def test_pack_cameras_layout():
    from luciddreamer_amd import cameras, filter3d
    cams = cameras.lookaround_path(64, 48, n_views=3)
    p = filter3d.pack_cameras(cams, "cpu")
    assert p.shape == (3, 20) and p.dtype == torch.float32
    for n, c in enumerate(cams):
        assert torch.equal(p[n, :16].reshape(4, 4), c.world_view_transform)
        assert abs(float(p[n, 16]) - 64 / (2 * math.tan(c.FoVx / 2))) < 1e-5
        assert abs(float(p[n, 17]) - 48 / (2 * math.tan(c.FoVy / 2))) < 1e-5
        assert float(p[n, 18]) == 64 and float(p[n, 19]) == 48
    assert filter3d.pack_cameras([], "cpu").shape == (0, 20)


def test_host_tensors_and_wrong_lengths_raise():
    from luciddreamer_amd import filter3d
    s, o = torch.zeros(10, 3), torch.zeros(10, 1)
    with pytest.raises(ValueError, match="recompute"):
        filter3d.apply(s, o, torch.zeros(9, 1))
    with pytest.raises(RuntimeError, match="HIP device"):
        filter3d.apply(s, o, torch.zeros(10, 1))
    with pytest.raises(RuntimeError, match="HIP device"):
        filter3d.compute_filter_3d(torch.zeros(10, 3), torch.zeros(2, 20))
    m = types.SimpleNamespace(_scaling=s, _opacity=o, _xyz=torch.zeros(10, 3))
    with pytest.raises(ValueError, match="recompute"):
        filter3d.filtered(m, torch.zeros(11, 1))
    with pytest.raises(RuntimeError, match="HIP device"):
        filter3d.filtered(m, torch.zeros(10, 1))


def test_example_has_the_switch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_loop_example_filter3d", os.path.join(ROOT, "examples", "train_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.default_args().filter3d is False
    args = mod.make_parser().parse_args(["--filter3d"])
    assert args.filter3d is True and args.antialiasing is False
    assert "Independent of --antialiasing" in mod.HELP["filter3d"] and "Independent of --antialiasing" in mod.__doc__
