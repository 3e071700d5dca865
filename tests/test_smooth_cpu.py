"""CPU: the references of the edge-aware smoothness term (tests/smooth_ref.py) and the boundary of the new entry points:
lr_smooth_args against its ctypes mirror, every refusal that sits in front of the first HIP call, the exports, smooth.hip in the
library's gfx950 code object, and the Python module's own refusals.  The GPU tests (tests/test_gpu_smooth.py) rely on what is
asserted here: the float64 reference has the properties of the definition, its analytic gradient is the derivative of its value,
and the float32 restatements count the same terms."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import smooth_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference's own properties -----------------------------------------------------------------------------------------
def test_a_tilted_plane_has_no_second_order_term_and_a_first_order_one():
    H, W = 9, 11
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    plane = (2.0 + 0.25 * x + 0.125 * y)[None]                       # exactly representable: the second difference is exactly 0
    r2 = sr.reference(plane, order=2, positive_only=True)
    assert r2["count"] == H * (W - 2) + (H - 2) * W and r2["value"] == 0.0 and not r2["grad"].any()      # sign(0) = 0
    r1 = sr.reference(plane, order=1, positive_only=True, weight=1.0)
    assert r1["count"] == H * (W - 1) + (H - 1) * W
    assert r1["value"] == pytest.approx((H * (W - 1) * 0.25 + (H - 1) * W * 0.125) / (H * W), rel=1e-14)
    inv = sr.reference(plane, order=2, space="inverse", positive_only=True)
    assert inv["value"] > 0                                           # 1 / plane is not a plane


@pytest.mark.parametrize("channels", [1, 3])
def test_a_term_across_the_guide_edge_is_down_weighted(channels):
    H, W, gamma, step = 4, 8, 3.0, 0.5
    ramp = np.broadcast_to(np.arange(W, dtype=np.float64), (1, H, W)) + 1.0          # every horizontal difference is 1
    guide = np.zeros((channels, H, W))
    guide[:, :, W // 2:] = step
    r = sr.reference(ramp, guide, order=1, gamma=gamma, weight=1.0)
    want = (H * (W - 2) + H * np.exp(-gamma * step)) / (H * W)        # one pair per row straddles the edge
    assert r["value"] == pytest.approx(want, rel=1e-14)
    # order 2 on x^2: every second difference is 2; the two triples per row that touch the edge are both gated
    r = sr.reference(ramp ** 2, guide, order=2, gamma=gamma, weight=1.0)
    want = 2.0 * (H * (W - 4) + 2 * H * np.exp(-gamma * step)) / (H * W)
    assert r["value"] == pytest.approx(want, rel=1e-14)
    # the pixel left of the edge: its gradient is k (w_left_pair - w_edge_pair) = k (1 - exp(-gamma step)) at order 1
    g = sr.reference(ramp, guide, order=1, gamma=gamma, weight=1.0)["grad"]
    assert g[0, 1, W // 2 - 1] == pytest.approx((1.0 - np.exp(-gamma * step)) / (H * W), rel=1e-12)


def test_validity_rules():
    d = np.full((1, 3, 4), 2.0)
    d[0, 1, 1] = 0.0
    full = 3 * 3 + 2 * 4
    assert sr.reference(d, order=1, positive_only=False)["count"] == full            # a zero is a value like any other ...
    assert sr.reference(d, order=1, positive_only=True)["count"] == full - 4         # ... unless it means "no surface"
    d[0, 1, 1] = np.nan
    assert sr.reference(d, order=1)["count"] == full - 4
    d[0, 1, 1] = 2.0
    mask = np.ones((3, 4))
    mask[1, 1] = np.nan
    r = sr.reference(d, mask=mask, order=1)
    assert r["count"] == full - 4 and not r["grad"][0, 1, 1]
    guide = np.zeros((1, 3, 4))
    guide[0, 0, 0] = np.nan                                            # a NaN in the guide excludes the terms across it
    assert sr.reference(d, guide, order=1)["count"] == full - 2
    assert sr.reference(d, guide, order=2)["count"] == (3 * 2 + 1 * 4) - 2
    guide[0, 0, 0] = np.inf                                            # ... and so does an infinite value: its weight at
    for gamma in (0.0, 2.0):                                           # gamma = 0 would be exp(-(0 inf)) = NaN
        r = sr.reference(d, guide, order=1, gamma=gamma)
        assert r["count"] == full - 2 and np.isfinite(r["value"]) and np.isfinite(r["grad"]).all()
    # INVERSE space: a subnormal depth is > 0 and finite, but its float32 reciprocal is not: the pixel is invalid there only
    tiny = np.full((1, 3, 4), 2.0, np.float32)
    tiny[0, 1, 1] = np.float32(1e-40)
    with np.errstate(over="ignore"):
        assert tiny[0, 1, 1] > 0 and np.isinf(np.float32(1) / tiny[0, 1, 1])
    assert sr.reference(tiny, order=1, positive_only=True)["count"] == full
    for f in (sr.reference, sr.restate32):
        r = f(tiny, order=1, space="inverse", positive_only=True)
        assert r["count"] == full - 4 and np.isfinite(r["value"]) and np.isfinite(r["grad"]).all() and not r["grad"][0, 1, 1]
    for shape, order in (((1, 1, 1), 1), ((1, 2, 2), 2), ((1, 1, 2), 2)):
        r = sr.reference(np.ones(shape), order=order)
        assert r["count"] == 0 and r["value"] == 0.0 and not r["grad"].any()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("what", ["depth", "inverse", "vectors"])
def test_central_differences_match_the_analytic_gradient(order, what):
    """Random data: every |difference| is far above the step, so no kink is crossed."""
    H, W = 5, 7
    case = sr.make_case(H, W, 11, "rand")
    x = (case["vectors"] if what == "vectors" else case["depth"][None]).astype(np.float64)
    kw = dict(guide=case["texture"], mask=case["mask"], order=order, space="inverse" if what == "inverse" else "depth",
              positive_only=what != "vectors")
    r = sr.reference(x, **kw)
    assert r["count"] > 0
    eps, worst = 1e-6, 0.0
    for idx in np.ndindex(*x.shape):
        hi, lo = x.copy(), x.copy()
        hi[idx] += eps
        lo[idx] -= eps
        fd = (sr.reference(hi, **kw)["value"] - sr.reference(lo, **kw)["value"]) / (2 * eps)
        worst = max(worst, abs(fd - r["grad"][idx]))
    print(f"order {order} {what}: max|finite difference - analytic| {worst:.2e} of max|g| {np.abs(r['grad']).max():.2e}")
    assert worst <= 1e-7 * np.abs(r["grad"]).max()


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (2, 9), (9, 2), (3, 3), (5, 7), (16, 16), (67, 131)])
@pytest.mark.parametrize("order", [1, 2])
def test_restatements_count_what_the_reference_counts(H, W, order):
    case = sr.make_case(H, W, 1000 * H + W, "rand")
    for space in ("depth", "inverse"):
        kw = dict(guide=case["guide"], mask=case["mask"], order=order, space=space, positive_only=True)
        r = sr.reference(case["depth"][None], **kw)
        a = sr.restate32(case["depth"][None], **kw)
        b = sr.restate32(case["depth"][None], gather="reverse", **kw)
        assert a["count"] == r["count"] == b["count"] and np.array_equal(a["counted_x"], r["counted_x"])
        assert abs(a["value"] - r["value"]) <= 1e-6
        assert not a["grad"][r["grad"] == 0].any() and not b["grad"][r["grad"] == 0].any()
        gmax = np.abs(r["grad"]).max()
        assert max(np.abs(a["grad"] - r["grad"]).max(), np.abs(b["grad"] - r["grad"]).max()) <= 1e-5 * gmax
    if (H, W) == (1, 2):
        assert sr.reference(case["depth"][None], order=1, positive_only=True)["count"] == 1
    if H * W >= 256:
        r = sr.reference(case["depth"][None], case["guide"], case["mask"], order=order, positive_only=True)
        assert 0.5 * 2 * H * W <= r["count"] < 2 * H * W and (r["grad"] == 0).any()


# ---- the argument struct (the method of tests/test_mesh_cpu.py) ---------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


def test_ctypes_structure_mirrors_the_header(tmp_path):
    from luciddreamer_amd import _lib
    S = _lib.SmoothArgs
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    members = [(f[0], getattr(S, f[0]).offset, getattr(S, f[0]).size) for f in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lucid_raster.h"\nint main(void)\n{\n'
                   '    printf("sizeof %zu\\n", sizeof(lr_smooth_args));\n'
                   '    printf("spaces %d %d\\n", LR_SMOOTH_DIRECT, LR_SMOOTH_INVERSE);\n' +
                   "".join(f'    printf("{n} %zu %zu\\n", offsetof(lr_smooth_args, {n}), sizeof(((lr_smooth_args*)0)->{n}));\n'
                           for n, _, _ in members) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(S)}"
    assert lines[1] == f"spaces {_lib.LR_SMOOTH_DIRECT} {_lib.LR_SMOOTH_INVERSE}"
    assert lines[2:2 + len(members)] == [f"{n} {o} {s}" for n, o, s in members]
    end = 0                                             # every member is mirrored: the fields tile the struct up to padding
    for n, o, s in members:
        assert 0 <= o - end < 8, n
        end = o + s
    assert 0 <= ctypes.sizeof(S) - end < 8
    assert [m[0] for m in members] == ["struct_bytes", "height", "width", "channels", "guide_channels", "map", "guide", "mask",
                                       "order", "space", "positive_only", "gamma", "weight", "upstream", "out", "dL_dmap",
                                       "workspace", "workspace_bytes", "stream"]


ENTRIES = ("lr_smooth_forward", "lr_smooth_backward")


def test_exports_and_declarations(L):
    from luciddreamer_amd import _lib
    header = open(os.path.join(ROOT, "include", "lucid_raster.h")).read()
    for name in ENTRIES + ("lr_smooth_workspace_bytes",):
        assert name in _lib.EXPORTS
        getattr(L, name)                                 # exported by the built library
        assert name + "(" in header
    assert "typedef struct lr_smooth_args" in header
    assert L.lr_smooth_workspace_bytes(1080, 1920) > 0
    assert L.lr_smooth_workspace_bytes(0, 16) == 0 and L.lr_smooth_workspace_bytes(65536, 65536) == 0
    assert L.lr_smooth_workspace_bytes(1, 1) > 0         # no term, but a legal call


def test_struct_bytes_is_checked_before_anything_else(L):
    from luciddreamer_amd import _lib
    for name in ENTRIES:
        entry = getattr(L, name)
        assert entry(None) == _lib.LR_ERR_INVALID_ARG
        a = _lib.SmoothArgs(height=-1)                   # everything else is wrong as well
        assert a.struct_bytes == ctypes.sizeof(_lib.SmoothArgs)
        for wrong in (0, a.struct_bytes - 8, a.struct_bytes + 8):
            a.struct_bytes = wrong
            assert entry(a) == _lib.LR_ERR_INVALID_ARG, wrong
            assert b"struct_bytes" in L.lr_last_error() and name.encode() in L.lr_last_error()


def _valid(L, name, **over):
    """A call of `name` that passes every check (never made: each case breaks one thing); pointers are one small host buffer."""
    from luciddreamer_amd import _lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    f = dict(height=16, width=16, channels=1, guide_channels=3, map=p, guide=p, mask=p, order=2, space=_lib.LR_SMOOTH_INVERSE,
             positive_only=1, gamma=2.0, weight=1.0)
    if name == "lr_smooth_forward":
        f.update(out=p, workspace=p, workspace_bytes=1 << 20)
    else:
        f.update(dL_dmap=p)
    f.update(over)
    if f.get("workspace_bytes") == -1:
        n = L.lr_smooth_workspace_bytes(f["height"], f["width"])
        assert n > 0
        f["workspace_bytes"] = n - 1
    a = _lib.SmoothArgs(**f)
    a._keep = buf
    return a


def _refusals():
    dims = b"height, width must be positive"
    guide = b"guide_channels must be 1 or 3 with a guide, 0 without one"
    out = []
    for name in ENTRIES:
        out += [(name, "zero_height", dict(height=0), dims), (name, "negative_width", dict(width=-3), dims),
                (name, "too_many_pixels", dict(height=65536, width=65536), dims),
                (name, "dims_before_pointers", dict(width=0, map=None), dims),
                (name, "null_map", dict(map=None), b"map is required"),
                (name, "channels_0", dict(channels=0), b"channels must be 1..4"),
                (name, "channels_5", dict(channels=5, space=0), b"channels must be 1..4"),
                (name, "guide_channels_2", dict(guide_channels=2), guide),
                (name, "guide_channels_0_with_guide", dict(guide_channels=0), guide),
                (name, "guide_channels_without_guide", dict(guide=None), guide),
                (name, "order_0", dict(order=0), b"order must be 1 or 2"), (name, "order_3", dict(order=3), b"order must be 1 or 2"),
                (name, "space_2", dict(space=2), b"space must be LR_SMOOTH_DIRECT or LR_SMOOTH_INVERSE"),
                (name, "space_negative", dict(space=-1), b"space must be LR_SMOOTH_DIRECT or LR_SMOOTH_INVERSE"),
                (name, "positive_only_2", dict(positive_only=2), b"positive_only must be 0 or 1"),
                (name, "inverse_of_three_channels", dict(channels=3), b"LR_SMOOTH_INVERSE needs channels = 1 and positive_only"),
                (name, "inverse_without_positive_only", dict(positive_only=0), b"LR_SMOOTH_INVERSE needs channels = 1 and positive_only")]
        for k in ("gamma", "weight"):
            for bad in (-0.5, float("nan"), float("inf")):
                out.append((name, f"{k}_{bad}", {k: bad}, k.encode() + b" must be finite and >= 0"))
    out += [("lr_smooth_forward", "null_out", dict(out=None), b"out and workspace are required"),
            ("lr_smooth_forward", "null_workspace", dict(workspace=None), b"out and workspace are required"),
            ("lr_smooth_forward", "workspace_one_byte_short", dict(workspace_bytes=-1), b"workspace too small (lr_smooth_workspace_bytes)"),
            ("lr_smooth_forward", "workspace_zero", dict(workspace_bytes=0), b"workspace too small (lr_smooth_workspace_bytes)"),
            ("lr_smooth_forward", "pointers_before_workspace", dict(workspace_bytes=-1, out=None), b"out and workspace are required"),
            ("lr_smooth_backward", "null_dL_dmap", dict(dL_dmap=None), b"dL_dmap is required")]
    return out


REFUSALS = _refusals()


@pytest.mark.parametrize("name,case,over,fragment", REFUSALS, ids=[f"{n}-{c}" for n, c, _, _ in REFUSALS])
def test_argument_checks_without_a_device(L, name, case, over, fragment):
    """Every pointer of the call is HOST memory and the machine may have no device: a check that came behind a launch would fault
    or report a HIP error instead of the message."""
    from luciddreamer_amd import _lib
    rc = getattr(L, name)(_valid(L, name, **over))
    assert rc == _lib.LR_ERR_INVALID_ARG
    assert fragment in L.lr_last_error() and name.encode() in L.lr_last_error(), L.lr_last_error()


def test_python_module_refuses_before_any_library_call(monkeypatch):
    import torch
    import luciddreamer_amd
    from luciddreamer_amd import _lib, smooth
    assert luciddreamer_amd.smooth is smooth

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    d = torch.ones(8, 8)
    for call in (lambda: smooth.depth_smoothness(d), lambda: smooth.depth_smoothness(d[None], torch.ones(3, 8, 8)),
                 lambda: smooth.map_smoothness(torch.ones(3, 8, 8)), lambda: smooth.smoothness_count(d, depth=True)):
        with pytest.raises(RuntimeError, match=r"luciddreamer_amd\.smooth\..*HIP device"):
            call()
    # dtype, rank, shape and channel count are judged before the device, so CPU tensors reach every one of them
    ones = lambda *shape, dtype=torch.float32: torch.ones(shape, dtype=dtype)
    refusals = [(lambda: smooth.depth_smoothness(ones(8, 8, dtype=torch.float64)), "depth_smoothness: depth must be float32"),
                (lambda: smooth.depth_smoothness(ones(8, 8, dtype=torch.float16)), "depth_smoothness: depth must be float32"),
                (lambda: smooth.depth_smoothness(ones(8)), r"depth_smoothness: depth \(8,\) must be \[1,H,W\] or \[H,W\]"),
                (lambda: smooth.depth_smoothness(ones(1, 1, 8, 8)), r"depth_smoothness: depth .* must be \[1,H,W\] or \[H,W\]"),
                (lambda: smooth.depth_smoothness(ones(3, 8, 8)), r"depth_smoothness: depth .* with C in \(1,\)"),
                (lambda: smooth.map_smoothness(ones(8, 8)), r"map_smoothness: x .* must be \[C,H,W\]"),
                (lambda: smooth.map_smoothness(ones(5, 8, 8)), r"map_smoothness: x .* with C in \(1, 2, 3, 4\)"),
                (lambda: smooth.map_smoothness(ones(3, 8, 8, dtype=torch.int32)), "map_smoothness: x must be float32"),
                (lambda: smooth.smoothness_count(ones(2, 8, 8), depth=True), r"smoothness_count: depth .* with C in \(1,\)"),
                (lambda: smooth.smoothness_count("depth"), "smoothness_count: x must be a tensor")]
    for call, fragment in refusals:
        with pytest.raises(RuntimeError, match=r"luciddreamer_amd\.smooth\." + fragment):
            call()
    like = ones(1, 8, 8)
    for bad, channels, fragment in ((ones(2, 8, 8), (1, 3), r"image .* with C in \(1, 3\)"),
                                    (ones(3, 8, 8, dtype=torch.float64), (1, 3), "image must be float32"),
                                    (ones(3, 8, 9), (1, 3), "image .* must have the H, W of the map"),
                                    (ones(8, 8), (1, 3), r"image .* must be \[C,H,W\]")):
        with pytest.raises(RuntimeError, match=r"luciddreamer_amd\.smooth\.depth_smoothness: " + fragment):
            smooth._image(bad, "image", "depth_smoothness", channels, like)
    with pytest.raises(RuntimeError, match=r"luciddreamer_amd\.smooth\.depth_smoothness: mask .* must have the H, W of the map"):
        smooth._plane(ones(4, 8), "mask", "depth_smoothness", like)
    for kw, fragment in ((dict(order=3), "order must be 1 or 2"), (dict(space="disparity"), 'space must be "depth" or "inverse"')):
        with pytest.raises(RuntimeError, match=r"luciddreamer_amd\.smooth\.depth_smoothness: " + fragment):
            smooth._inputs(like, None, None, **dict(dict(order=1, space="depth", positive_only=True, gamma=1.0,
                                                         what="depth_smoothness"), **kw))


# ---- smooth.hip compiles for gfx950 and is in the library ---------------------------------------------------------------------
def test_smooth_hip_is_built_for_gfx950(L):
    from luciddreamer_amd import build
    from tests.test_normals_cpu import _gfx950_code_objects
    assert "smooth.hip" in build.SOURCES and "-ffp-contract=off" in build.SOURCES["smooth.hip"]
    assert os.path.exists(os.path.join(build.CSRC, "smooth.hip"))
    blob = b"".join(_gfx950_code_objects(build.LIB_PATH))
    assert blob, "no gfx950 code object in the library"
    for kernel in (b"12k_smooth_fwdILi1EE", b"12k_smooth_fwdILi2EE", b"14k_smooth_final", b"12k_smooth_bwdILi1EE",
                   b"12k_smooth_bwdILi2EE"):
        assert kernel in blob, kernel.decode()


def test_example_loop_has_the_three_flags_and_their_defaults():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_loop_example_smooth", os.path.join(ROOT, "examples", "train_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    d = mod.default_args()
    assert d.depth_smoothness == 0.0 and d.smoothness_order == 1 and d.smoothness_space == "depth"
    a = mod.make_parser().parse_args(["--depth-smoothness", "0.1", "--smoothness-order", "2", "--smoothness-space", "inverse"])
    assert a.depth_smoothness == 0.1 and a.smoothness_order == 2 and a.smoothness_space == "inverse"
    for bad in (["--smoothness-order", "3"], ["--smoothness-space", "disparity"]):
        with pytest.raises(SystemExit):
            mod.make_parser().parse_args(bad)
    with pytest.raises(SystemExit):                    # the multi-view step has no smoothness term of its own
        mod.train(mod.default_args(multi_view=2, depth_smoothness=0.1))
