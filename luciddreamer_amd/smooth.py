"""Edge-aware smoothness of a rendered map on the MI355X (include/lucid_raster.h, lr_smooth_args; INTEGRATION.md 2s,
DESIGN.md 4b-SMO).

    loss = depth_smoothness(depth, image)                        # first-order smoothness of a depth map, gated by image edges
    loss = depth_smoothness(depth, image, order=2, space="inverse")      # second order, on 1 / depth
    loss = map_smoothness(normals, image, mask=hole_mask)       # the same on a [C,H,W] map, e.g. a rendered normal map
    n = smoothness_count(depth, image, depth=True)              # the number of terms that counted

The regulariser of the Monodepth lineage, DNGaussian and MonoGS: the L1 norm of the map's first or second differences, each
term weighted by exp(-gamma |difference of the guide image|) so that the map may jump where the image has an edge.  It holds a
rendered depth smooth in the regions that one estimated depth map supervises and no second view constrains.  HIP in both
directions (luciddreamer_amd/csrc/smooth.hip), no CPU or PyTorch fallback, no atomics (bit-repeatable), no host
synchronisation.
"""
import ctypes

import torch

from . import _lib
from .loss import _weight, _ws_bytes

_SPACES = {"depth": _lib.LR_SMOOTH_DIRECT, "inverse": _lib.LR_SMOOTH_INVERSE}


def _refuse(what, text):
    raise RuntimeError(f"luciddreamer_amd.smooth.{what}: {text}")


def _image(t, name, what, channels, like=None):
    """A float32 device image [C,H,W] with C in `channels`, contiguous; with `like`, of its H, W and device."""
    if not isinstance(t, torch.Tensor):
        _refuse(what, f"{name} must be a tensor")
    if t.dtype != torch.float32:
        _refuse(what, f"{name} must be float32, got {t.dtype}")
    if t.dim() != 3 or t.shape[0] not in channels:
        _refuse(what, f"{name} {tuple(t.shape)} must be [C,H,W] with C in {tuple(channels)}")
    if like is not None and t.shape[-2:] != like.shape[-2:]:
        _refuse(what, f"{name} {tuple(t.shape)} must have the H, W of the map {tuple(like.shape)}")
    if not t.is_cuda:
        _refuse(what, f"{name} must be on a HIP device (no CPU path)")
    if like is not None and t.device != like.device:
        _refuse(what, f"{name} must be on the device of the map, {like.device}")
    return t.contiguous()


def _plane(t, name, what, like=None):
    """A float32 device plane [1,H,W] or [H,W] as a contiguous [1,H,W]."""
    if isinstance(t, torch.Tensor) and t.dim() == 2:
        t = t[None]
    elif isinstance(t, torch.Tensor) and t.dim() != 3:
        _refuse(what, f"{name} {tuple(t.shape)} must be [1,H,W] or [H,W]")
    return _image(t, name, what, (1,), like)


def _call(fn, what, dev, **fields):
    """fn(lr_smooth_args of `fields` and the current stream of dev) with dev the current HIP device; a refusal raises as `what`."""
    with _lib.on_device(dev):
        a = _lib.SmoothArgs(stream=torch.cuda.current_stream(dev).cuda_stream, **fields)
        rc = fn(ctypes.byref(a))
    if rc < 0:
        _lib.raise_for(rc, what)


def _inputs(x, image, mask, order, space, positive_only, gamma, what):
    """(fields of lr_smooth_args shared by the forward and the backward, the tensors they point into); x is [C,H,W]."""
    if order not in (1, 2):
        _refuse(what, f"order must be 1 or 2, got {order!r}")
    if space not in _SPACES:
        _refuse(what, f'space must be "depth" or "inverse", got {space!r}')
    fields = dict(height=int(x.shape[-2]), width=int(x.shape[-1]), channels=int(x.shape[0]), map=x.data_ptr(), order=int(order),
                  space=_SPACES[space], positive_only=1 if positive_only else 0, gamma=float(gamma))
    keep = [x]
    if image is not None:
        g = _image(image, "image", what, (1, 3), x)
        fields.update(guide=g.data_ptr(), guide_channels=int(g.shape[0]))
        keep.append(g)
    if mask is not None:
        m = _plane(mask, "mask", what, x)
        fields.update(mask=m.data_ptr())
        keep.append(m)
    return fields, keep


def _forward(x, fields, weight, what):
    """One lr_smooth_forward: out {loss, count}."""
    dev = x.device
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    ws = torch.empty((_ws_bytes("lr_smooth_workspace_bytes", fields["height"], fields["width"]),), dtype=torch.uint8, device=dev)
    _call(_lib.lib().lr_smooth_forward, what, dev, out=out.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
          weight=float(weight), **fields)
    return out


def _as_map(t, as_depth, what):
    """The checked, contiguous [C,H,W] form of the first argument."""
    return _plane(t, "depth", what) if as_depth else _image(t, "x", what, (1, 2, 3, 4))


class _Smoothness(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, image, mask, order, space, as_depth, gamma, weight, what):
        x = _as_map(t, as_depth, what)
        fields, keep = _inputs(x, image, mask, order, space, as_depth, gamma, what)
        out = _forward(x, fields, weight, what)
        ctx.save_for_backward(*keep)
        ctx.fields, ctx.weight, ctx.what, ctx.in_shape = fields, float(weight), what, t.shape
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x = ctx.saved_tensors[0]
        up = _weight(grad_out, x.device)
        grad = torch.empty_like(x)
        _call(_lib.lib().lr_smooth_backward, ctx.what + " backward", x.device, upstream=up.data_ptr(), dL_dmap=grad.data_ptr(),
              weight=ctx.weight, **ctx.fields)
        return (grad.view(ctx.in_shape),) + (None,) * 8


def depth_smoothness(depth, image=None, *, order=1, space="depth", gamma=1.0, weight=1.0, mask=None):
    """weight * sum over the counted terms of exp(-gamma a_t) |D_t| / (H*W): the edge-aware smoothness of a depth map [1,H,W] or
    [H,W] (the rasterizer's depth or median depth; 0 = no surface).  order=1: D is the difference of two horizontal or vertical
    neighbours; order=2: the second difference of three.  space="inverse": on 1 / depth.  image: optional guide [3,H,W] or
    [1,H,W] (the target or rendered colour, plain data); a is the mean over its channels of the absolute difference across the
    term (order 2: the larger of the two sides), so a term across an image edge hardly counts; without it every weight is 1.
    mask: optional [1,H,W] or [H,W] plane; a pixel whose value is not > 0 is left out (a selector: it is never multiplied in).
    A term counts when all of its pixels are finite, > 0 and selected; the sum is divided by ALL pixels -- smoothness_count
    gives the number of terms that counted, for renormalising.  One HIP pass and a one-workgroup reduction forward (double
    differences and sums, fixed order), one gather pass backward that recomputes weights and signs (lr_smooth_forward /
    lr_smooth_backward).  Gradients flow to `depth` only: `image` and `mask` are read as plain data, so an image that requires a
    gradient (a rendered colour passed undetached) gets none from this term, and the term has no second derivative."""
    return _Smoothness.apply(depth, image, mask, order, space, True, gamma, weight, "depth_smoothness")


def map_smoothness(x, image=None, *, order=1, gamma=1.0, weight=1.0, mask=None):
    """depth_smoothness on a map [C,H,W] of 1 to 4 channels, e.g. a rendered normal map (return_normals=True): the term of a
    pair or triple is the sum over the channels of |D|.  A pixel is valid when all of its channels are finite and the mask
    selects it -- no sign test, so a normal map with a hole mask works.  Gradients flow to `x` only."""
    return _Smoothness.apply(x, image, mask, order, "depth", False, gamma, weight, "map_smoothness")


def smoothness_count(x, image=None, *, order=1, space="depth", mask=None, depth=False):
    """The number of terms that count in map_smoothness of these inputs or, with depth=True, in depth_smoothness of them: a
    0-dim device tensor without a gradient, for renormalising (loss * H * W / count) and logging."""
    what = "smoothness_count"
    with torch.no_grad():
        m = _as_map(x.detach() if isinstance(x, torch.Tensor) else x, depth, what)
        fields, keep = _inputs(m, image, mask, order, space if depth else "depth", depth, 0.0, what)
        return _forward(m, fields, 1.0, what)[1]
