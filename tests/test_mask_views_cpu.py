"""CPU: mask supervision in the multi-view step -- the C-ABI surface (header, exports, pure host workspace sizes), the float64
restatement of the masked colour loss and the alpha hole term against their torch definitions, content_mask, and the argument
checks of ViewBatch, which must raise before any device (or the library) is touched."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mask_loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lr_masked_l1_dssim_forward", "lr_masked_l1_dssim_backward", "lr_alpha_hole_workspace_bytes", "lr_alpha_hole_forward",
       "lr_alpha_hole_backward", "lr_views_workspace_bytes", "lr_views_accumulate", "lr_views_check")
# the multi-view step is ONE entry point over lr_views_args with three LR_VIEWS_* flags; the positional per-mode forms are gone
FLAGS = {"LR_VIEWS_LOSS": 1, "LR_VIEWS_DEPTH_LOSS": 2, "LR_VIEWS_MASK_LOSS": 4}
RETIRED = ("lr_views_accumulate_alpha", "lr_views_train_mask_workspace_bytes", "lr_views_train_mask_accumulate",
           "lr_views_train_mask_check", "lr_views_accumulate_depth", "lr_views_train_depth_workspace_bytes",
           "lr_views_train_depth_accumulate", "lr_views_train_depth_check", "lr_views_train_workspace_bytes",
           "lr_views_train_accumulate", "lr_views_train_check")


@pytest.fixture(scope="module")
def built_lib():
    from luciddreamer_amd import build
    return build.build()


def _header():
    text = open(os.path.join(ROOT, "include", "lucid_raster.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared():
    text = _header()
    return set(re.findall(r"^(?:int|size_t) (lr_[a-z0-9_]+)\(", text, flags=re.M))


def test_header_declares_the_mask_entry_points():
    names = _declared()
    for n in NEW:
        assert n in names, n
    text = _header()
    assert re.search(r"typedef struct lr_views_args \{.*?\} lr_views_args;", text, flags=re.S)
    for flag, value in FLAGS.items():
        assert re.search(rf"^#define {flag}\s+{value}u\s*$", text, flags=re.M), flag
    for n in RETIRED:
        assert n not in names and not re.search(rf"\b{n}\b", text), n


def test_library_exports_the_mask_entry_points(built_lib):
    L = ctypes.CDLL(built_lib)
    from luciddreamer_amd import _lib
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS, n
    for n in RETIRED:
        assert not hasattr(L, n), n
        assert n not in _lib.EXPORTS, n
    assert (_lib.LR_VIEWS_LOSS, _lib.LR_VIEWS_DEPTH_LOSS, _lib.LR_VIEWS_MASK_LOSS) == tuple(FLAGS.values())


def test_mask_workspace_sizes_are_pure_host_functions(built_lib):
    from luciddreamer_amd import _lib
    L = _lib.lib()
    LOSS, DEPTH, MASK = _lib.LR_VIEWS_LOSS, _lib.LR_VIEWS_DEPTH_LOSS, _lib.LR_VIEWS_MASK_LOSS
    for P, W, H, cap in ((1, 16, 16, 1000), (25_000, 256, 160, 400_000), (1_000_000, 1920, 1080, 30_000_000)):
        for n in (1, 2, 3, 4):
            dep = L.lr_views_workspace_bytes(P, W, H, cap, n, LOSS | DEPTH)
            msk = L.lr_views_workspace_bytes(P, W, H, cap, n, LOSS | MASK)
            # the slot grows by the alpha gradient image (and the hole term's partials) behind the train-depth slot
            assert msk >= dep + n * W * H * 4, (P, W, H, n)
            assert msk % 256 == 0
            # the existing layouts are unchanged
            assert 0 <= L.lr_views_workspace_bytes(P, W, H, cap, n, 0) <= L.lr_views_workspace_bytes(P, W, H, cap, n, LOSS) <= dep
            # a mask step's slot always has the depth part
            assert L.lr_views_workspace_bytes(P, W, H, cap, n, LOSS | DEPTH | MASK) == msk
            # the mask or depth part without the colour loss, or an unknown bit, is no layout
            for bad in (MASK, DEPTH, DEPTH | MASK, LOSS | 8, 1 << 31):
                assert L.lr_views_workspace_bytes(P, W, H, cap, n, bad) == 0, bad
    for H, W in ((16, 16), (257, 511), (512, 512), (1080, 1920)):
        b = L.lr_alpha_hole_workspace_bytes(H, W)
        assert b >= math.ceil(H * W / 2048) * 8 and b % 256 == 0
    assert L.lr_alpha_hole_workspace_bytes(0, 16) == 0 and L.lr_alpha_hole_workspace_bytes(16, -1) == 0
    assert L.lr_alpha_hole_workspace_bytes(65536, 65536) == 0


@pytest.mark.parametrize("H,W", [(16, 16), (29, 37), (1, 1)])
@pytest.mark.parametrize("kind", ["soft", "binary"])
def test_numpy_restatement_of_the_masked_colour_loss(H, W, kind):
    g = torch.Generator().manual_seed(H * 100 + W)
    gt = torch.rand(3, H, W, generator=g, dtype=torch.float64)
    img = (0.6 * gt + 0.4 * torch.rand(3, H, W, generator=g, dtype=torch.float64)).requires_grad_(True)
    m = mask_loss_ref.make_mask(H, W, seed=H + W, kind=kind).double()
    loss = mask_loss_ref.torch_masked_l1_dssim(img, gt, m, 0.2)
    loss.backward()
    o = mask_loss_ref.numpy_masked_l1_dssim(img.detach().numpy(), gt.numpy(), m.numpy(), 0.2)
    assert abs(float(loss.detach()) - o["loss"]) <= 1e-12
    assert np.abs(img.grad.numpy() - o["grad"]).max() <= 1e-12 * max(1.0, np.abs(o["grad"]).max())
    # nothing reaches a hole
    assert not np.any(o["grad"][:, m.numpy()[0] == 0])


def test_all_ones_mask_is_the_plain_loss():
    from oracle import loss_oracle
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(3, 24, 20, generator=g, dtype=torch.float64)
    img = torch.rand(3, 24, 20, generator=g, dtype=torch.float64)
    o = mask_loss_ref.numpy_masked_l1_dssim(img.numpy(), gt.numpy(), np.ones((24, 20)), 0.2)
    p = loss_oracle.l1_dssim(img.numpy(), gt.numpy(), 0.2)
    assert o["loss"] == p["loss"] and np.array_equal(o["grad"], p["grad"])


@pytest.mark.parametrize("H,W", [(16, 16), (257, 511), (1, 1)])
@pytest.mark.parametrize("weight", [1.0, 0.3])
def test_numpy_restatement_of_the_alpha_hole_term(H, W, weight):
    g = torch.Generator().manual_seed(H + 7 * W)
    alpha = torch.rand(1, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    m = mask_loss_ref.make_mask(H, W, seed=W, kind="soft").double()
    loss = mask_loss_ref.torch_alpha_hole(alpha, m, weight)
    loss.backward()
    want, grad = mask_loss_ref.numpy_alpha_hole(alpha.detach().numpy(), m.numpy(), weight)
    assert abs(float(loss.detach()) - want) <= 1e-12 * max(1.0, abs(want))
    assert np.allclose(alpha.grad.numpy(), grad, rtol=1e-14, atol=0)


def test_content_mask_rebuilds_the_holes():
    from luciddreamer_amd.loss import content_mask
    gt = torch.rand(3, 8, 9) + 0.01
    gt[:, 2:4, 3:7] = 0                       # a hole: every channel exact zero
    gt[1, 6, 0] = 0                           # one channel zero: still content
    m = content_mask(gt)
    assert m.shape == (1, 8, 9) and m.dtype == torch.float32
    assert not m[0, 2:4, 3:7].any() and float(m.sum()) == 8 * 9 - 8 and float(m[0, 6, 0]) == 1.0


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


@pytest.mark.parametrize("case", ["alpha_grads_with_targets", "masks_with_grads", "weight_without_masks", "negative_weight",
                                  "nan_weight", "inf_weight", "short_alpha_grads", "bad_alpha_shape", "short_masks",
                                  "bad_mask_shape", "alphas_without_alpha", "alphas_with_colour_train", "cpu_alpha_outputs",
                                  "bad_alphas_shape", "double_masks"])
def test_view_batch_mask_argument_errors(no_library, case):
    from luciddreamer_amd import parallel
    n, W, H = 3, 32, 24
    cams = _cams(n, W, H)
    img = [torch.zeros(3, H, W)] * n
    one = [torch.zeros(1, H, W)] * n
    kw = dict(bg=torch.zeros(3), binning_capacity=1000, sh_degree=0)
    args = {
        "alpha_grads_with_targets": dict(grad_colors=None, targets=img, grad_alphas=one),
        "masks_with_grads": dict(grad_colors=img, masks=one),
        "weight_without_masks": dict(grad_colors=None, targets=img, alpha_weight=0.5),
        "negative_weight": dict(grad_colors=None, targets=img, masks=one, alpha_weight=-0.1),
        "nan_weight": dict(grad_colors=None, targets=img, masks=one, alpha_weight=float("nan")),
        "inf_weight": dict(grad_colors=None, targets=img, masks=one, alpha_weight=float("inf")),
        "short_alpha_grads": dict(grad_colors=img, grad_alphas=one[:2]),
        "bad_alpha_shape": dict(grad_colors=img, grad_alphas=[torch.zeros(1, W, H)] * n),
        "short_masks": dict(grad_colors=None, targets=img, masks=one[:1]),
        "bad_mask_shape": dict(grad_colors=None, targets=img, masks=[torch.zeros(3, H, W)] * n),
        "alphas_without_alpha": dict(grad_colors=img, alphas=one),
        "alphas_with_colour_train": dict(grad_colors=None, targets=img, alphas=one),
        "cpu_alpha_outputs": dict(grad_colors=img, grad_alphas=one, alphas=one),
        "bad_alphas_shape": dict(grad_colors=img, grad_alphas=one, alphas=[torch.zeros(2, H, W)] * n),
        "double_masks": dict(grad_colors=None, targets=img, masks=[torch.zeros(1, H, W, dtype=torch.float64)] * n),
    }[case]
    grad_colors = args.pop("grad_colors")
    with pytest.raises(ValueError):
        parallel.ViewBatch(cams, grad_colors, **kw, **args)
