"""CPU: the references of the normals from depth (tests/normal_ref.py) against each other, and the boundary of the new entry points:
lr_normals_args against its ctypes mirror, every refusal that sits in front of the first HIP call, the exports, and normals.hip
in the library's gfx950 code object.  The GPU tests (tests/test_gpu_normals.py) rely on what is asserted here: the lifted-point
definition in float64 and the header's closed form agree to 1e-12, every case counts enough pixels, and each float32 calibrator
passes the per-pixel judge against the other."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import normal_ref as nr, rowbar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX, TY = nr.TAN

# the GPU test's shapes that a CPU test can afford (600 x 900 is left to the GPU test: see the calibrator test below)
SHAPES = [(3, 3), (5, 7), (16, 16), (67, 131), (257, 511)]
DEGENERATE = [(2, 9), (9, 2)]


def _seed(H, W):
    return 1000 * H + W


def _target(case, mode):
    return dict(target_depth=case["depth_b"]) if mode == "consistency" else dict(target_normals=case["target_normals"])


@pytest.mark.parametrize("H,W", SHAPES + DEGENERATE)
@pytest.mark.parametrize("kind,mode", [("smooth", "target"), ("smooth", "consistency"), ("rand", "target")])
def test_lifted_points_and_closed_form_agree_in_float64(H, W, kind, mode):
    case = nr.make_case(H, W, _seed(H, W), kind)
    for with_weight in (True, False):
        pw = case["pixel_weight"] if with_weight else None
        r = nr.reference(case, TX, TY, mode, with_weight, 0.7)
        c = nr.closed_form(case["depth"], TX, TY, np.float64, pixel_weight=pw, weight=0.7, **_target(case, mode))
        assert np.array_equal(r["valid"], c["valid"]) and np.array_equal(r["counted"], c["counted"]) and r["count"] == c["count"]
        assert np.abs(r["normals"] - c["normals"]).max() <= 1e-12
        assert not c["normals"][:, ~c["valid"]].any()
        assert abs(r["value"] - c["value"]) <= 1e-12
        for k in ("grad", "grad_target") if mode == "consistency" else ("grad",):
            assert np.abs(r[k] - c[k]).max() <= 1e-12 * np.abs(r[k]).max(), k
        if (H, W) in DEGENERATE:
            assert r["count"] == 0 and r["value"] == 0.0 and not r["grad"].any() and not c["grad"].any() and not c["normals"].any()
        else:
            # the condition of the GPU test: enough of the pixels that can count do
            frac = nr.counted_fraction(r, H, W)
            print(f"{H}x{W} {kind} {mode} weight plane {with_weight}: {r['count']} counted, {frac:.2f} of the interior")
            assert frac >= nr.MIN_COUNTED and np.abs(r["grad"]).max() > 0
            for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):        # no normal reads a corner
                assert r["grad"][y, x] == 0.0 and c["grad"][y, x] == 0.0


@pytest.mark.parametrize("H,W", SHAPES)
def test_vjp_of_the_normals_agrees_in_float64(H, W):
    case = nr.make_case(H, W, _seed(H, W), "smooth")
    Gn = np.random.default_rng(7).standard_normal((3, H, W)).astype(np.float32)
    r = nr.reference_vjp(case["depth"], Gn, TX, TY)
    c = nr.closed_form_vjp(case["depth"], Gn, TX, TY, np.float64)
    assert np.abs(r).max() > 0 and np.abs(r - c).max() <= 1e-12 * np.abs(r).max()


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind,mode", [("smooth", "target"), ("smooth", "consistency"), ("rand", "target")])
def test_each_float32_calibrator_passes_the_judge_against_the_other(H, W, kind, mode):
    """The two calibrators of the GPU test's gradient bar -- the header's gather order and its reverse, both float32 -- each held
    to rowbar.judge (pixels as rows, no fragile rows) with the OTHER as the only calibrator: harsher than the GPU test, which
    gives the judge both.  At 600 x 900 one calibrator alone is not enough (measured: 1 to 2 of 540 000 pixels, whose four terms
    cancel to 1e-3 of their size, where one order happens to round four times better than the other), which is why the judge
    gets two; that shape runs on the GPU only."""
    case = nr.make_case(H, W, _seed(H, W), kind)
    r = nr.reference(case, TX, TY, mode, True, 0.7)
    kw = dict(pixel_weight=case["pixel_weight"], weight=0.7, **_target(case, mode))
    a = nr.closed_form(case["depth"], TX, TY, np.float32, order="WENS", **kw)
    b = nr.closed_form(case["depth"], TX, TY, np.float32, order="SNEW", **kw)
    assert a["count"] == r["count"] and np.array_equal(a["valid"], r["valid"]) and abs(a["value"] - r["value"]) <= 1e-7
    col = lambda g: g.reshape(-1, 1)
    for k in ("grad", "grad_target") if mode == "consistency" else ("grad",):
        for got, cal in ((a, b), (b, a)):
            rep = rowbar.judge(col(got[k]), col(r[k]), [col(cal[k])])
            assert not rep["failed"], (k, rep["failed"][:3])
        e32 = max(np.abs(a[k] - r[k]).max(), np.abs(b[k] - r[k]).max()) / np.abs(r[k]).max()
        print(f"{H}x{W} {kind} {mode} {k}: float32 restatements within {e32:.2e} of the gradient's maximum")


def test_doubling_the_depth_leaves_the_float32_normals_bit_identical():
    case = nr.make_case(67, 131, 5, "rand")
    n1, v1 = nr.closed_normals(case["depth"], TX, TY, np.float32)
    n2, v2 = nr.closed_normals(case["depth"] * np.float32(2), TX, TY, np.float32)
    assert v1.any() and np.array_equal(v1, v2) and np.array_equal(n1.view(np.uint32), n2.view(np.uint32))


def test_the_closed_form_keeps_its_digits_where_the_lifted_form_loses_them():
    """A smooth 1080-line depth map in float32: the lifted-point definition subtracts neighbouring points whose rays differ by
    2 tan / W, the closed form only subtracts depths."""
    H, W = 270, 1920                                     # a band of a 1080p frame: the rays' spacing is what matters
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    d = (4.0 + 0.8 * np.sin(0.01 * x) + 0.5 * np.cos(0.012 * y)).astype(np.float32)
    ty = TX * 1080 / 1920 * H / 1080
    n64, _ = nr.closed_normals(d, TX, ty, np.float64)
    n32, _ = nr.closed_normals(d, TX, ty, np.float32)
    f = np.float32
    u = (f(2) * f(TX) / f(W)) * (np.arange(W).astype(f) + f(0.5)) - f(TX)
    v = (f(2) * f(ty) / f(H)) * (np.arange(H).astype(f) + f(0.5)) - f(ty)
    P = np.stack([d * u[None, :], d * v[:, None], d])
    c = np.cross(P[:, 2:, 1:-1] - P[:, :-2, 1:-1], P[:, 1:-1, 2:] - P[:, 1:-1, :-2], axis=0)
    lifted = c / np.sqrt((c * c).sum(0))
    assert lifted.dtype == np.float32
    e_closed = np.abs(n32 - n64)[:, 1:-1, 1:-1].max()
    e_lifted = np.abs(lifted - n64[:, 1:-1, 1:-1]).max()
    print(f"float32 normals against float64 on a smooth {H}x{W} depth map: closed form {e_closed:.2e}, lifted points {e_lifted:.2e}")
    assert e_closed <= 16 * 2.0 ** -24 and e_lifted > 20 * e_closed


# ---- the argument struct (the method of tests/test_views_args_cpu.py) -----------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


def test_ctypes_structure_mirrors_the_header(tmp_path):
    from luciddreamer_amd import _lib
    S = _lib.NormalsArgs
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    members = [(f[0], getattr(S, f[0]).offset, getattr(S, f[0]).size) for f in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lucid_raster.h"\nint main(void)\n{\n'
                   '    printf("sizeof %zu\\n", sizeof(lr_normals_args));\n' +
                   "".join(f'    printf("{n} %zu %zu\\n", offsetof(lr_normals_args, {n}), sizeof(((lr_normals_args*)0)->{n}));\n'
                           for n, _, _ in members) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(S)}"
    assert lines[1:1 + len(members)] == [f"{n} {o} {s}" for n, o, s in members]
    end = 0                                             # every member is mirrored: the fields tile the struct up to padding
    for n, o, s in members:
        assert 0 <= o - end < 8, n
        end = o + s
    assert 0 <= ctypes.sizeof(S) - end < 8


ENTRIES = ("lr_depth_normals", "lr_depth_normals_backward", "lr_normal_loss_forward", "lr_normal_loss_backward")
LOSS = ("lr_normal_loss_forward", "lr_normal_loss_backward")


def test_exports(L):
    from luciddreamer_amd import _lib
    for name in ENTRIES + ("lr_normals_workspace_bytes",):
        assert name in _lib.EXPORTS
        getattr(L, name)                                 # exported by the built library
    assert L.lr_normals_workspace_bytes(1080, 1920) > 0
    assert L.lr_normals_workspace_bytes(0, 16) == 0 and L.lr_normals_workspace_bytes(65536, 65536) == 0
    assert L.lr_normals_workspace_bytes(2, 2) > 0        # no valid pixel, but a legal call


def test_struct_bytes_is_checked_before_anything_else(L):
    from luciddreamer_amd import _lib
    for name in ENTRIES:
        entry = getattr(L, name)
        assert entry(None) == _lib.LR_ERR_INVALID_ARG
        a = _lib.NormalsArgs(height=-1)                  # everything else is wrong as well
        assert a.struct_bytes == ctypes.sizeof(_lib.NormalsArgs)
        for wrong in (0, a.struct_bytes - 8, a.struct_bytes + 8):
            a.struct_bytes = wrong
            assert entry(a) == _lib.LR_ERR_INVALID_ARG, wrong
            assert b"struct_bytes" in L.lr_last_error() and name.encode() in L.lr_last_error()


def _valid(L, name, **over):
    """A call of `name` that passes every check (never made: each case breaks one thing); pointers are one small host buffer."""
    from luciddreamer_amd import _lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    f = dict(height=16, width=16, tan_fovx=0.7, tan_fovy=0.45, depth=p)
    if name == "lr_depth_normals":
        f.update(out_normals=p)
    elif name == "lr_depth_normals_backward":
        f.update(dL_dnormals=p, dL_ddepth=p)
    else:
        f.update(target_normals=p, weight=1.0)
        if name == "lr_normal_loss_forward":
            f.update(out=p, workspace=p, workspace_bytes=1 << 20)
        else:
            f.update(dL_ddepth=p)
    for k, v in over.items():
        f[k] = p if v == "ptr" else v
    if f.get("workspace_bytes") == -1:
        n = L.lr_normals_workspace_bytes(f["height"], f["width"])
        assert n > 0
        f["workspace_bytes"] = n - 1
    a = _lib.NormalsArgs(**f)
    a._keep = buf
    return a


def _refusals():
    dims = b"height, width must be positive"
    tan = b"tan_fovx and tan_fovy must be finite and > 0"
    one = b"exactly one of target_normals and target_depth"
    out = []
    for name in ENTRIES:
        out += [(name, "zero_height", dict(height=0), dims), (name, "negative_width", dict(width=-3), dims),
                (name, "too_many_pixels", dict(height=65536, width=65536), dims),
                (name, "dims_before_pointers", dict(width=0, depth=None), dims),
                (name, "null_depth", dict(depth=None), b"depth is required")]
        for k in ("tan_fovx", "tan_fovy"):
            for bad in (0.0, -0.5, float("nan"), float("inf")):
                out.append((name, f"{k}_{bad}", {k: bad}, tan))
    out += [("lr_depth_normals", "null_out_normals", dict(out_normals=None), b"out_normals is required"),
            ("lr_depth_normals_backward", "null_dL_dnormals", dict(dL_dnormals=None), b"dL_dnormals and dL_ddepth are required"),
            ("lr_depth_normals_backward", "null_dL_ddepth", dict(dL_ddepth=None), b"dL_dnormals and dL_ddepth are required")]
    for name in LOSS:
        out += [(name, "both_targets", dict(target_depth="ptr"), one), (name, "no_target", dict(target_normals=None), one)]
        for bad in (-0.5, float("nan"), float("inf")):
            out.append((name, f"weight_{bad}", dict(weight=bad), b"weight must be finite and >= 0"))
    out += [("lr_normal_loss_forward", "null_out", dict(out=None), b"out and workspace are required"),
            ("lr_normal_loss_forward", "null_workspace", dict(workspace=None), b"out and workspace are required"),
            ("lr_normal_loss_forward", "workspace_one_byte_short", dict(workspace_bytes=-1), b"workspace too small (lr_normals_workspace_bytes)"),
            ("lr_normal_loss_forward", "workspace_zero", dict(workspace_bytes=0), b"workspace too small (lr_normals_workspace_bytes)"),
            ("lr_normal_loss_forward", "pointers_before_workspace", dict(workspace_bytes=-1, out=None), b"out and workspace are required"),
            ("lr_normal_loss_backward", "null_dL_ddepth", dict(dL_ddepth=None), b"dL_ddepth is required"),
            ("lr_normal_loss_backward", "target_gradient_without_target_depth", dict(dL_dtarget_depth="ptr"),
             b"dL_dtarget_depth goes with target_depth only")]
    return out


REFUSALS = _refusals()


@pytest.mark.parametrize("name,case,over,fragment", REFUSALS, ids=[f"{n}-{c}" for n, c, _, _ in REFUSALS])
def test_argument_checks_without_a_device(L, name, case, over, fragment):
    from luciddreamer_amd import _lib
    rc = getattr(L, name)(_valid(L, name, **over))
    assert rc == _lib.LR_ERR_INVALID_ARG
    assert fragment in L.lr_last_error() and name.encode() in L.lr_last_error(), L.lr_last_error()


def test_python_module_refuses_host_tensors_and_wrong_shapes():
    import torch
    import luciddreamer_amd
    from luciddreamer_amd import normals
    assert luciddreamer_amd.normals is normals
    d = torch.ones(8, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        normals.depth_normals(d, (0.7, 0.45))
    with pytest.raises(RuntimeError, match="HIP device"):
        normals.normal_loss(d, torch.ones(3, 8, 8), (0.7, 0.45))
    with pytest.raises(RuntimeError, match="HIP device"):
        normals.normal_consistency(d, d, (0.7, 0.45))
    for bad in ((0.0, 0.45), (0.7, float("nan")), "xy", 3.0):
        with pytest.raises(RuntimeError):
            normals._tans(bad)
    from luciddreamer_amd import cameras
    import math
    cam = cameras.identity_camera(64, 48)
    assert normals._tans(cam) == (math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
    rgb = normals.normals_to_rgb(torch.tensor([[[0.0]], [[0.0]], [[-1.0]]]))
    assert rgb.flatten().tolist() == [0.5, 0.5, 1.0]


# ---- normals.hip compiles for gfx950 and is in the library -----------------------------------------------------------------------
def _gfx950_code_objects(path):
    data = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, pos = [], 0
    while True:
        i = data.find(magic, pos)
        if i < 0:
            return out
        pos = i + 1
        n = struct.unpack_from("<Q", data, i + 24)[0]
        p = i + 32
        if n > 16:
            continue
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tl]
            p += tl
            if b"gfx950" in triple and size:
                out.append(data[i + off:i + off + size])


def test_normals_hip_is_built_for_gfx950(L):
    from luciddreamer_amd import build
    assert "normals.hip" in build.SOURCES and "-ffp-contract=off" in build.SOURCES["normals.hip"]
    assert os.path.exists(os.path.join(build.CSRC, "normals.hip"))
    blob = b"".join(_gfx950_code_objects(build.LIB_PATH))
    assert blob, "no gfx950 code object in the library"
    for kernel in (b"15k_depth_normals", b"19k_depth_normals_bwd", b"19k_normal_loss_final", b"17k_normal_loss_fwdILb0EE",
                   b"17k_normal_loss_fwdILb1EE", b"17k_normal_loss_bwdILb0EE", b"17k_normal_loss_bwdILb1EE"):
        assert kernel in blob, kernel.decode()


def test_example_loop_has_the_two_flags_and_their_defaults():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_loop_example_normals", os.path.join(ROOT, "examples", "train_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    d = mod.default_args()
    assert d.normal_weight == 0.0 and d.normal_consistency == 0.0
    a = mod.make_parser().parse_args(["--normal-weight", "0.05", "--normal-consistency", "0.1"])
    assert a.normal_weight == 0.05 and a.normal_consistency == 0.1
    with pytest.raises(SystemExit):                    # the multi-view step has no normal term of its own
        mod.train(mod.default_args(multi_view=2, normal_weight=0.05))
