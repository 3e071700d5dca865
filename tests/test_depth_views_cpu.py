"""CPU: depth supervision in the multi-view step -- the C-ABI surface (header, exports, pure host workspace sizes), the float64
restatement of the masked depth L1 against its torch definition, and the argument checks of ViewBatch / ViewStreams.run_view,
which must raise before any device (or the library) is touched."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import depth_l1_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lr_views_workspace_bytes", "lr_views_accumulate", "lr_views_check", "lr_depth_l1_workspace_bytes", "lr_depth_l1_forward",
       "lr_depth_l1_backward")
# the multi-view step is ONE entry point over lr_views_args with three LR_VIEWS_* flags; the positional per-mode forms are gone
FLAGS = {"LR_VIEWS_LOSS": 1, "LR_VIEWS_DEPTH_LOSS": 2, "LR_VIEWS_MASK_LOSS": 4}
RETIRED = ("lr_views_accumulate_depth", "lr_views_train_depth_workspace_bytes", "lr_views_train_depth_accumulate",
           "lr_views_train_depth_check", "lr_views_train_workspace_bytes", "lr_views_train_accumulate", "lr_views_train_check",
           "lr_views_accumulate_alpha", "lr_views_train_mask_workspace_bytes", "lr_views_train_mask_accumulate",
           "lr_views_train_mask_check")


@pytest.fixture(scope="module")
def built_lib():
    from luciddreamer_amd import build
    return build.build()


def _header():
    text = open(os.path.join(ROOT, "include", "lucid_raster.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared():
    text = _header()
    return set(re.findall(r"^(?:int|size_t) (lr_[a-z0-9_]+)\($", text, flags=re.M) +
               re.findall(r"^(?:int|size_t) (lr_[a-z0-9_]+)\(", text, flags=re.M))


def test_header_declares_the_depth_entry_points():
    names = _declared()
    for n in NEW:
        assert n in names, n
    text = _header()
    assert re.search(r"typedef struct lr_views_args \{.*?\} lr_views_args;", text, flags=re.S)
    for flag, value in FLAGS.items():
        assert re.search(rf"^#define {flag}\s+{value}u\s*$", text, flags=re.M), flag
    for n in RETIRED:
        assert n not in names and not re.search(rf"\b{n}\b", text), n


def test_library_exports_the_depth_entry_points(built_lib):
    L = ctypes.CDLL(built_lib)
    from luciddreamer_amd import _lib
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS, n
    for n in RETIRED:
        assert not hasattr(L, n), n
        assert n not in _lib.EXPORTS, n
    assert (_lib.LR_VIEWS_LOSS, _lib.LR_VIEWS_DEPTH_LOSS, _lib.LR_VIEWS_MASK_LOSS) == tuple(FLAGS.values())


def test_depth_workspace_sizes_are_pure_host_functions(built_lib):
    from luciddreamer_amd import _lib
    L = _lib.lib()
    LOSS, DEPTH = _lib.LR_VIEWS_LOSS, _lib.LR_VIEWS_DEPTH_LOSS
    for P, W, H, cap in ((1, 16, 16, 1000), (25_000, 256, 160, 400_000), (1_000_000, 1920, 1080, 30_000_000)):
        for n in (1, 2, 3, 4):
            base = L.lr_views_workspace_bytes(P, W, H, cap, n, LOSS)
            dep = L.lr_views_workspace_bytes(P, W, H, cap, n, LOSS | DEPTH)
            # the slot grows by the depth gradient image (and the loss partials); nothing else changes
            assert dep >= base + n * W * H * 4, (P, W, H, n)
            assert dep % 256 == 0
            assert 0 <= L.lr_views_workspace_bytes(P, W, H, cap, n, 0) <= base
            # the depth part without the colour loss, or an unknown bit, is no layout
            assert L.lr_views_workspace_bytes(P, W, H, cap, n, DEPTH) == 0
            assert L.lr_views_workspace_bytes(P, W, H, cap, n, LOSS | 8) == 0
    # the depth L1 workspace: one double per 2048-pixel workgroup, 256-byte aligned; 0 for an impossible size
    for H, W in ((16, 16), (257, 511), (512, 512), (1080, 1920)):
        b = L.lr_depth_l1_workspace_bytes(H, W)
        assert b >= math.ceil(H * W / 2048) * 8 and b % 256 == 0
    assert L.lr_depth_l1_workspace_bytes(0, 16) == 0 and L.lr_depth_l1_workspace_bytes(16, -1) == 0
    assert L.lr_depth_l1_workspace_bytes(65536, 65536) == 0


@pytest.mark.parametrize("H,W", [(16, 16), (257, 511), (33, 7), (1, 1)])
@pytest.mark.parametrize("weight", [1.0, 0.25])
def test_numpy_restatement_matches_torch_definition(H, W, weight):
    depth, target = depth_l1_ref.make_pair(H, W, seed=H * 1000 + W, lead=(1,))
    d = depth.double().requires_grad_(True)
    loss = depth_l1_ref.torch_depth_l1(d, target.double(), weight)
    loss.backward()
    want, grad = depth_l1_ref.numpy_depth_l1(depth.numpy(), target.numpy(), weight)
    assert math.isfinite(want)
    assert abs(float(loss.detach()) - want) <= 1e-12 * max(1.0, abs(want))
    assert np.array_equal(d.grad.numpy(), grad)


def test_restatement_ties_masks_and_nan():
    depth = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    target = torch.tensor([[1.0, 0.0, -1.0, float("nan"), 4.0, 7.0]])       # tie, masked x2, NaN, above, below
    loss, grad = depth_l1_ref.numpy_depth_l1(depth.numpy(), target.numpy(), 2.0)
    assert loss == pytest.approx(2.0 * (0 + 1 + 1) / 6)
    assert np.array_equal(grad, np.array([[0, 0, 0, 0, 1, -1]]) * 2.0 / 6)
    d = depth.double().requires_grad_(True)
    t = depth_l1_ref.torch_depth_l1(d, target.double(), 2.0)
    t.backward()
    assert float(t.detach()) == pytest.approx(loss) and np.array_equal(d.grad.numpy(), grad)
    # all masked: zero loss, zero gradient
    loss0, grad0 = depth_l1_ref.numpy_depth_l1(depth.numpy(), np.zeros((1, 6)), 1.0)
    assert loss0 == 0.0 and not grad0.any()


def _cams(n, W=32, H=24):
    eye = torch.eye(4)
    return [SimpleNamespace(world_view_transform=eye, full_proj_transform=eye, camera_center=torch.zeros(3), FoVx=1.0, FoVy=0.8,
                            image_width=W, image_height=H) for _ in range(n)]


@pytest.fixture
def no_library(monkeypatch):
    """The argument checks must come first: loading the library (or any device work) on the way is a failure here."""
    from luciddreamer_amd import _lib

    def refuse():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.mark.parametrize("case", ["depth_grads_with_targets", "depth_targets_with_grads", "weight_without_targets",
                                  "negative_weight", "nan_weight", "short_depth_grads", "bad_depth_shape",
                                  "short_depth_targets", "depths_with_colour_train", "cpu_depth_outputs", "bad_depths_shape"])
def test_view_batch_depth_argument_errors(no_library, case):
    from luciddreamer_amd import parallel
    n, W, H = 3, 32, 24
    cams = _cams(n, W, H)
    img = [torch.zeros(3, H, W)] * n
    dep = [torch.zeros(1, H, W)] * n
    kw = dict(bg=torch.zeros(3), binning_capacity=1000, sh_degree=0)
    args = {
        "depth_grads_with_targets": dict(grad_colors=None, targets=img, grad_depths=dep),
        "depth_targets_with_grads": dict(grad_colors=img, depth_targets=dep),
        "weight_without_targets": dict(grad_colors=None, targets=img, depth_weight=0.5),
        "negative_weight": dict(grad_colors=None, targets=img, depth_targets=dep, depth_weight=-0.1),
        "nan_weight": dict(grad_colors=None, targets=img, depth_targets=dep, depth_weight=float("nan")),
        "short_depth_grads": dict(grad_colors=img, grad_depths=dep[:2]),
        "bad_depth_shape": dict(grad_colors=img, grad_depths=[torch.zeros(1, W, H)] * n),
        "short_depth_targets": dict(grad_colors=None, targets=img, depth_targets=dep[:1]),
        "depths_with_colour_train": dict(grad_colors=None, targets=img, depths=dep),
        "cpu_depth_outputs": dict(grad_colors=img, grad_depths=dep, depths=dep),
        "bad_depths_shape": dict(grad_colors=img, depths=[torch.zeros(2, H, W)] * n),
    }[case]
    grad_colors = args.pop("grad_colors")
    with pytest.raises(ValueError):
        parallel.ViewBatch(cams, grad_colors, **kw, **args)


def test_run_view_depth_argument_errors(no_library):
    """grad_depth with the depth switch off (the autograd paths would drop it) or with a backward_fn: ValueError, before
    forward_fn runs or any stream is touched."""
    from luciddreamer_amd import config, parallel
    vs = parallel.ViewStreams.__new__(parallel.ViewStreams)          # no streams: nothing may reach them
    called = []
    fwd = lambda: called.append(1)
    g, gd = torch.zeros(3, 8, 8), torch.zeros(1, 8, 8)
    assert not config.depth_gradient()
    with pytest.raises(ValueError, match="set_depth_gradient"):
        vs.run_view(fwd, grad_output=g, grad_depth=gd)
    config.set_depth_gradient(True)
    try:
        with pytest.raises(ValueError):
            vs.run_view(fwd, backward_fn=lambda out: None, grad_depth=gd)
    finally:
        config.set_depth_gradient(False)
    assert not called
