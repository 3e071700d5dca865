"""CPU: the Pearson depth loss -- the float64 restatement (tests/depth_pearson_ref.py) against torch autograd of the definition
and under a * t + b, the C-ABI surface (header layout of lr_views_args with depth_loss as its last member, exports, host-side
workspace sizes) and every argument check that sits in front of the first HIP call: of the three lr_depth_pearson_* entry points,
of lr_views_accumulate's depth_loss, of ViewBatch(depth_loss=) and of loss.depth_pearson, plus the example's flag."""
import ctypes
import math
import os
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import depth_pearson_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lr_depth_pearson_workspace_bytes", "lr_depth_pearson_forward", "lr_depth_pearson_backward")


@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 16), (257, 511)])
def test_closed_form_gradient_equals_autograd_of_the_definition(H, W):
    depth, target = ref.make_pair(H, W, seed=H + W)
    loss, rho, grad = ref.numpy_depth_pearson(depth.numpy(), target.numpy(), 0.7)
    d = depth.double().requires_grad_(True)
    t = ref.torch_depth_pearson(d, target, 0.7)
    t.backward()
    assert 0.5 < rho < 1.0 and loss == pytest.approx(0.7 * (1.0 - rho), abs=1e-15)
    assert abs(float(t.detach()) - loss) <= 1e-12
    want = d.grad.numpy()
    assert np.abs(want).max() > 0
    assert np.abs(grad - want).max() <= 1e-10 * np.abs(want).max()
    with np.errstate(invalid="ignore"):
        assert not grad[~(target.numpy() > 0)].any()                  # masked and NaN targets: exactly no gradient


@pytest.mark.parametrize("a,b", [(2.0, 0.0), (0.5, 3.0), (1.0, 0.25), (37.0, 11.0)])
def test_restatement_is_invariant_under_scale_and_shift(a, b):
    depth, target = ref.make_pair(64, 48, seed=5)
    d, t = depth.double().numpy(), target.double().numpy()
    with np.errstate(invalid="ignore"):
        t2 = np.where(t > 0, a * t + b, t)                             # float64: the transform itself is not rounded
    l0, r0, g0 = ref.numpy_depth_pearson(d, t)
    l1, r1, g1 = ref.numpy_depth_pearson(d, t2)
    assert abs(l0 - l1) <= 1e-12 and abs(r0 - r1) <= 1e-12
    assert np.abs(g0 - g1).max() <= 1e-10 * np.abs(g0).max()


def test_restatement_degenerate_inputs_are_zero():
    d = np.linspace(1.0, 2.0, 12).reshape(3, 4)
    t = np.linspace(2.0, 5.0, 12).reshape(3, 4) ** 2
    one = np.zeros_like(t)
    one[1, 2] = 3.0
    for dd, tt in ((d, np.zeros_like(t)), (d, np.full_like(t, np.nan)), (d, one), (np.full_like(d, 4.0), t), (d, np.full_like(t, 2.5))):
        loss, rho, grad = ref.numpy_depth_pearson(dd, tt, 2.0)
        assert loss == 0.0 and rho == 0.0 and not grad.any() and np.isfinite(grad).all()
    loss, rho, grad = ref.numpy_depth_pearson(d, t, 2.0)
    assert 0 < loss < 0.2 and grad.any()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_views_args_layout_with_depth_loss_as_the_last_member(tmp_path):
    from luciddreamer_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    names = [f[0] for f in _lib.ViewsArgs._fields_]
    assert names[-1] == "depth_loss" and names[-2] == "stream"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lucid_raster.h"\nint main(void)\n{\n'
                   '    printf("sizeof %zu\\n", sizeof(lr_views_args));\n' +
                   "".join(f'    printf("{n} %zu %zu\\n", offsetof(lr_views_args, {n}), sizeof(((lr_views_args*)0)->{n}));\n'
                           for n in names) +
                   '    printf("flags %u %d %d\\n", LR_VIEWS_DEPTH_PEARSON, LR_DEPTH_LOSS_L1, LR_DEPTH_LOSS_PEARSON);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(_lib.ViewsArgs)}"
    want = [f"{n} {getattr(_lib.ViewsArgs, n).offset} {getattr(_lib.ViewsArgs, n).size}" for n in names]
    assert lines[1:1 + len(names)] == want
    assert lines[1 + len(names)] == f"flags {_lib.LR_VIEWS_DEPTH_PEARSON} {_lib.LR_DEPTH_LOSS_L1} {_lib.LR_DEPTH_LOSS_PEARSON}"
    assert (_lib.LR_VIEWS_DEPTH_PEARSON, _lib.LR_DEPTH_LOSS_L1, _lib.LR_DEPTH_LOSS_PEARSON) == (16, 0, 1)
    # the member lies behind everything the struct held before, and the struct grew with it: a caller built without it has
    # another sizeof and is turned away by the struct_bytes check
    f, s = _lib.ViewsArgs.depth_loss, _lib.ViewsArgs.stream
    assert f.offset == s.offset + s.size and ctypes.sizeof(_lib.ViewsArgs) > f.offset >= ctypes.sizeof(_lib.ViewsArgs) - 8
    assert ctypes.sizeof(_lib.ViewsArgs) == s.offset + s.size + 8


def test_exports_and_host_side_sizes(L):
    from luciddreamer_amd import _lib, loss
    for n in NEW:
        assert hasattr(L, n) and n in _lib.EXPORTS, n
    assert callable(loss.depth_pearson) and callable(loss.depth_correlation)
    for H, W in ((16, 16), (257, 511), (600, 900), (1080, 1920)):
        b = L.lr_depth_pearson_workspace_bytes(H, W)
        # six doubles per 2048-pixel workgroup and the coefficient record behind them
        assert b >= math.ceil(H * W / 2048) * 48 + 48 and b % 256 == 0
        assert b > L.lr_depth_l1_workspace_bytes(H, W)
    assert L.lr_depth_pearson_workspace_bytes(0, 16) == 0 and L.lr_depth_pearson_workspace_bytes(16, -1) == 0
    assert L.lr_depth_pearson_workspace_bytes(65536, 65536) == 0
    LOSS, DEPTH, MASK, PEARSON = _lib.LR_VIEWS_LOSS, _lib.LR_VIEWS_DEPTH_LOSS, _lib.LR_VIEWS_MASK_LOSS, _lib.LR_VIEWS_DEPTH_PEARSON
    for P, W, H, cap in ((1, 16, 16, 1000), (25_000, 256, 160, 400_000), (1_000_000, 1920, 1080, 30_000_000)):
        grow = L.lr_depth_pearson_workspace_bytes(H, W) - L.lr_depth_l1_workspace_bytes(H, W)
        for n in (1, 2, 4):
            size = lambda parts: L.lr_views_workspace_bytes(P, W, H, cap, n, parts)
            for depth_part in (DEPTH, MASK, DEPTH | MASK):
                assert size(LOSS | depth_part | PEARSON) == size(LOSS | depth_part) + n * grow
            # the flag without a depth part, without the colour loss, and the value that is no flag
            assert size(LOSS | PEARSON) == 0 and size(PEARSON) == 0 and size(DEPTH | PEARSON) == 0
            assert size(LOSS | 8) == 0 and size(LOSS | DEPTH | 8) == 0 and size(LOSS | DEPTH | 32) == 0


def test_check_accepts_the_flag_only_with_a_depth_part(L):
    from luciddreamer_amd import _lib
    buf = (ctypes.c_char * 256)()
    LOSS, PEARSON = _lib.LR_VIEWS_LOSS, _lib.LR_VIEWS_DEPTH_PEARSON
    for bad in (PEARSON, LOSS | PEARSON, _lib.LR_VIEWS_DEPTH_LOSS | PEARSON, LOSS | 8, LOSS | _lib.LR_VIEWS_DEPTH_LOSS | 8):
        assert L.lr_views_check(ctypes.addressof(buf), 100, 16, 16, 1000, 2, bad, None) == _lib.LR_ERR_INVALID_ARG
        assert b"invalid parts" in L.lr_last_error()


def _pearson_args(**over):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    a = dict(H=16, W=16, depth=p, target=p, weight=1.0, out=p, upstream=None, ws=p, ws_bytes=1 << 20, grad=p, keep=buf)
    a.update(over)
    return a


FORWARD_BAD = {"null_depth": dict(depth=None), "null_target": dict(target=None), "null_out": dict(out=None),
               "null_workspace": dict(ws=None), "zero_height": dict(H=0), "negative_width": dict(W=-3),
               "too_many_pixels": dict(H=65536, W=65536), "workspace_too_small": dict(ws_bytes=64), "workspace_zero": dict(ws_bytes=0),
               "negative_weight": dict(weight=-0.5), "nan_weight": dict(weight=float("nan")), "inf_weight": dict(weight=float("inf"))}
BACKWARD_BAD = dict({k: v for k, v in FORWARD_BAD.items() if k != "null_out"}, null_grad=dict(grad=None))


@pytest.mark.parametrize("case", sorted(FORWARD_BAD))
def test_forward_argument_checks_without_a_device(L, case):
    from luciddreamer_amd import _lib
    a = _pearson_args(**FORWARD_BAD[case])
    rc = L.lr_depth_pearson_forward(a["H"], a["W"], a["depth"], a["target"], a["weight"], a["out"], a["ws"], a["ws_bytes"], None)
    assert rc == _lib.LR_ERR_INVALID_ARG and L.lr_last_error()


@pytest.mark.parametrize("case", sorted(BACKWARD_BAD))
def test_backward_argument_checks_without_a_device(L, case):
    from luciddreamer_amd import _lib
    a = _pearson_args(**BACKWARD_BAD[case])
    rc = L.lr_depth_pearson_backward(a["H"], a["W"], a["depth"], a["target"], a["weight"], a["upstream"], a["ws"], a["ws_bytes"],
                                     a["grad"], None)
    assert rc == _lib.LR_ERR_INVALID_ARG and L.lr_last_error()


def test_workspace_bound_is_the_size_query(L):
    """One byte short of lr_depth_pearson_workspace_bytes is refused by both entry points."""
    from luciddreamer_amd import _lib
    n = L.lr_depth_pearson_workspace_bytes(16, 16)
    a = _pearson_args(ws_bytes=n - 1)
    assert L.lr_depth_pearson_forward(16, 16, a["depth"], a["target"], 1.0, a["out"], a["ws"], n - 1, None) == _lib.LR_ERR_INVALID_ARG
    assert b"lr_depth_pearson_workspace_bytes" in L.lr_last_error()
    assert L.lr_depth_pearson_backward(16, 16, a["depth"], a["target"], 1.0, None, a["ws"], n - 1, a["grad"],
                                       None) == _lib.LR_ERR_INVALID_ARG
    assert b"lr_depth_pearson_workspace_bytes" in L.lr_last_error()


# ---- the multi-view step ----------------------------------------------------------------------------------------------------------
def test_views_accumulate_rejects_bad_depth_loss(L):
    from luciddreamer_amd import _lib
    from tests.test_views_args_cpu import TRAIN, _fake_step
    depth = dict(TRAIN, depth_targets="per_view", depth_weight=1.0)
    for fields, what in ((dict(depth, depth_loss=2), b"depth_loss"), (dict(depth, depth_loss=-1), b"depth_loss"),
                         (dict(TRAIN, depth_loss=1), b"depth_targets"), (dict(dL_dpix="per_view", depth_loss=1), b"depth_targets"),
                         (dict(TRAIN, masks="per_view", alpha_weight=1.0, depth_loss=1), b"depth_targets")):
        assert L.lr_views_accumulate(_fake_step(**fields)) == _lib.LR_ERR_INVALID_ARG, fields
        assert what in L.lr_last_error(), (fields, L.lr_last_error())
    # accepted values get as far as the workspace check
    for mode in (_lib.LR_DEPTH_LOSS_L1, _lib.LR_DEPTH_LOSS_PEARSON):
        assert L.lr_views_accumulate(_fake_step(**dict(depth, depth_loss=mode, workspace_bytes=4096))) == _lib.LR_ERR_INVALID_ARG
        assert b"workspace too small" in L.lr_last_error()
    # the selector is read behind the struct_bytes check: the size of the struct without the member is turned away
    a = _fake_step(**depth)
    a.struct_bytes = ctypes.sizeof(_lib.ViewsArgs) - 8
    assert L.lr_views_accumulate(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()


def _cams(n, W=32, H=24):
    eye = torch.eye(4)
    return [SimpleNamespace(world_view_transform=eye, full_proj_transform=eye, camera_center=torch.zeros(3), FoVx=1.0, FoVy=0.8,
                            image_width=W, image_height=H) for _ in range(n)]


def test_view_batch_depth_loss_argument(monkeypatch):
    from luciddreamer_amd import _lib, parallel

    def refuse():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)
    n, W, H = 2, 32, 24
    img, dep = [torch.zeros(3, H, W)] * n, [torch.zeros(1, H, W)] * n
    kw = dict(bg=torch.zeros(3), binning_capacity=1000, sh_degree=0)
    with pytest.raises(ValueError, match="depth_loss"):
        parallel.ViewBatch(_cams(n, W, H), None, targets=img, depth_targets=dep, depth_loss="huber", **kw)
    with pytest.raises(ValueError, match="depth_loss"):
        parallel.ViewBatch(_cams(n, W, H), None, targets=img, depth_targets=dep, depth_loss=None, **kw)
    with pytest.raises(ValueError, match="depth_targets"):
        parallel.ViewBatch(_cams(n, W, H), None, targets=img, depth_loss="pearson", **kw)
    with pytest.raises(ValueError, match="depth_targets"):
        parallel.ViewBatch(_cams(n, W, H), img, depth_loss="pearson", **kw)


def test_view_batch_passes_the_selector_and_the_parts(L):
    """Construction touches no device: the argument struct carries depth_loss and the parts carry the Pearson flag."""
    from luciddreamer_amd import _lib, parallel
    n, W, H = 2, 32, 24
    img, dep = [torch.zeros(3, H, W)] * n, [torch.zeros(1, H, W)] * n
    kw = dict(bg=torch.zeros(3), binning_capacity=1000, sh_degree=0, targets=img, depth_targets=dep)
    base = _lib.LR_VIEWS_LOSS | _lib.LR_VIEWS_DEPTH_LOSS
    for given, mode, parts in (({}, 0, base), (dict(depth_loss="l1"), 0, base),
                               (dict(depth_loss="pearson"), 1, base | _lib.LR_VIEWS_DEPTH_PEARSON)):
        b = parallel.ViewBatch(_cams(n, W, H), None, **kw, **given)
        assert b._args.depth_loss == mode and b.parts == parts and tuple(b.losses.shape) == (n, 4)
    assert (parallel.ViewBatch(_cams(n, W, H), None, **kw, depth_loss="pearson").workspace_bytes(100) >
            parallel.ViewBatch(_cams(n, W, H), None, **kw).workspace_bytes(100))


def test_depth_pearson_on_cpu_tensors_raises():
    from luciddreamer_amd import loss
    d, t = torch.rand(1, 8, 8), torch.rand(1, 8, 8) + 0.5
    with pytest.raises(RuntimeError, match="HIP device"):
        loss.depth_pearson(d.requires_grad_(True), t)
    with pytest.raises(RuntimeError, match="HIP device"):
        loss.depth_correlation(d, t)


def test_example_parser_accepts_the_flag():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_loop
    finally:
        sys.path.pop(0)
    ap = train_loop.make_parser()
    assert ap.parse_args([]).depth_loss == "l1" and ap.parse_args([]).depth_weight == 0.0
    a = ap.parse_args(["--multi-view", "4", "--depth-weight", "0.1", "--depth-loss", "pearson"])
    assert (a.depth_loss, a.depth_weight, a.multi_view) == ("pearson", 0.1, 4)
    with pytest.raises(SystemExit):
        ap.parse_args(["--depth-loss", "huber"])
    assert train_loop.default_args().depth_loss == "l1"
