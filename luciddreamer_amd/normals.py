"""Surface normals from a depth map and the fused normal losses on the MI355X (include/lucid_raster.h, lr_normals_args;
INTEGRATION.md 2l).

    n = depth_normals(depth, camera)                            # [3,H,W], differentiable in depth
    loss = normal_loss(depth, target_normals, camera)           # mean over all pixels of w (1 - n.t), t a monocular normal estimate
    loss = normal_consistency(depth, median_depth, camera)      # the same between the normals of two depth maps

The normal of a pixel is 2DGS's depth_to_normal -- the normalised cross product of the central differences of the lifted points,
oriented towards the camera -- in a closed form whose only cancellation is the depth difference itself.  Normals are the one
geometric quantity of an ESTIMATED depth map that does not depend on its unknown scale.  HIP in both directions
(luciddreamer_amd/csrc/normals.hip), no CPU or PyTorch fallback, no atomics (bit-repeatable), no host synchronisation.
"""
import ctypes
import math

import torch

from . import _lib
from .loss import _plane, _weight, _ws_bytes


def _tans(camera):
    """(tan_fovx, tan_fovy) of a MiniCam / reference camera (FoVx, FoVy) or of such a pair itself."""
    if hasattr(camera, "FoVx") and hasattr(camera, "FoVy"):
        tx, ty = math.tan(float(camera.FoVx) * 0.5), math.tan(float(camera.FoVy) * 0.5)
    else:
        try:
            tx, ty = camera
            tx, ty = float(tx), float(ty)
        except (TypeError, ValueError):
            raise RuntimeError("camera must have FoVx and FoVy, or be a (tan_fovx, tan_fovy) pair") from None
    if not (math.isfinite(tx) and math.isfinite(ty) and tx > 0 and ty > 0):
        raise RuntimeError(f"tan_fovx, tan_fovy must be finite and > 0, got {tx}, {ty}")
    return tx, ty


def _call(fn, what, dev, **fields):
    """fn(lr_normals_args of `fields` and the current stream of dev) with dev the current HIP device; a refusal raises as `what`."""
    with _lib.on_device(dev):
        a = _lib.NormalsArgs(stream=torch.cuda.current_stream(dev).cuda_stream, **fields)
        rc = fn(ctypes.byref(a))
    if rc < 0:
        _lib.raise_for(rc, what)


def _same_plane(t, name, what, like):
    """_plane of one H, W and device with the depth `like`."""
    p = _plane(t, name, what)
    if p.shape[-2:] != like.shape[-2:] or p.device != like.device:
        raise RuntimeError(f"{name} {tuple(t.shape)} must be [1,H,W] or [H,W] with the H, W and device of depth {tuple(like.shape)}")
    return p


def _normal_image(t, name, what, like):
    """A float32 device image [3,H,W] of the depth's H, W, contiguous."""
    if not t.is_cuda or t.device != like.device:
        raise RuntimeError(f"luciddreamer_amd.normals.{what}: {name} must be on the HIP device of depth (no CPU path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32")
    if t.dim() != 3 or t.shape[0] != 3 or t.shape[-2:] != like.shape[-2:]:
        raise RuntimeError(f"{name} {tuple(t.shape)} must be [3,H,W] with the H, W of depth {tuple(like.shape)}")
    return t.contiguous()


def _geometry(d, camera):
    tx, ty = _tans(camera)
    return dict(height=int(d.shape[-2]), width=int(d.shape[-1]), tan_fovx=tx, tan_fovy=ty)


class _DepthNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, camera):
        d = _plane(depth, "depth", "depth_normals")
        geo = _geometry(d, camera)
        out = torch.empty((3, geo["height"], geo["width"]), dtype=torch.float32, device=d.device)
        _call(_lib.lib().lr_depth_normals, "depth_normals", d.device, depth=d.data_ptr(), out_normals=out.data_ptr(), **geo)
        ctx.save_for_backward(d)
        ctx.geo, ctx.in_shape = geo, depth.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        d, = ctx.saved_tensors
        g = grad_out.to(torch.float32).contiguous()
        grad = torch.empty_like(d)
        _call(_lib.lib().lr_depth_normals_backward, "depth_normals backward", d.device, depth=d.data_ptr(), dL_dnormals=g.data_ptr(),
              dL_ddepth=grad.data_ptr(), **ctx.geo)
        return grad.view(ctx.in_shape), None


def depth_normals(depth, camera):
    """[3,H,W] unit normals of a depth map [1,H,W] or [H,W] (the rasterizer's depth or median depth; 0 = no surface), in view
    space (x right, y down, z forward), oriented towards the camera.  camera: a MiniCam / reference camera (FoVx, FoVy) or a
    (tan_fovx, tan_fovy) pair.  A pixel on the image border, or with a depth that is not > 0 (NaN included) at itself or one of
    its four neighbours, has the normal (0,0,0) and passes no gradient.  Differentiable in depth (lr_depth_normals /
    lr_depth_normals_backward): a gather, bit-repeatable."""
    return _DepthNormals.apply(depth, camera)


def _loss_inputs(depth, target_normals, target_depth, camera, pixel_weight, weight, what):
    """(d, fields of lr_normals_args shared by the loss forward and backward, the tensors they point into)."""
    d = _plane(depth, "depth", what)
    fields = _geometry(d, camera)
    fields.update(depth=d.data_ptr(), weight=float(weight))
    keep = [d]
    if target_normals is not None:
        t = _normal_image(target_normals, "target_normals", what, d)
        fields["target_normals"] = t.data_ptr()
    else:
        t = _same_plane(target_depth, "target depth", what, d)
        fields["target_depth"] = t.data_ptr()
    keep.append(t)
    if pixel_weight is not None:
        w = _same_plane(pixel_weight, "pixel_weight", what, d)
        fields["pixel_weight"] = w.data_ptr()
        keep.append(w)
    return d, fields, keep


def _loss_forward(depth, target_normals, target_depth, camera, pixel_weight, weight, what):
    """One lr_normal_loss_forward: (out {loss, count}, fields, keep)."""
    d, fields, keep = _loss_inputs(depth, target_normals, target_depth, camera, pixel_weight, weight, what)
    dev = d.device
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    ws = torch.empty((_ws_bytes("lr_normals_workspace_bytes", fields["height"], fields["width"]),), dtype=torch.uint8, device=dev)
    _call(_lib.lib().lr_normal_loss_forward, what, dev, out=out.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
          **fields)
    return out, fields, keep


class _NormalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, target_normals, camera, pixel_weight, weight):
        out, fields, keep = _loss_forward(depth, target_normals, None, camera, pixel_weight, weight, "normal_loss")
        ctx.save_for_backward(*keep)
        ctx.fields, ctx.in_shape = fields, depth.shape
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        d = ctx.saved_tensors[0]
        up = _weight(grad_out, d.device)
        grad = torch.empty_like(d)
        _call(_lib.lib().lr_normal_loss_backward, "normal_loss backward", d.device, upstream=up.data_ptr(), dL_ddepth=grad.data_ptr(),
              **ctx.fields)
        return grad.view(ctx.in_shape), None, None, None, None


def normal_loss(depth, target_normals, camera, pixel_weight=None, weight=1.0):
    """weight * sum over the counted pixels of w_p (1 - n_p . t_p) / (H*W): the cosine term of the depth's normals against a
    normal map (a monocular estimate).  depth [1,H,W] or [H,W]; target_normals [3,H,W], plain data in the convention of
    depth_normals, normalised in the kernel (a zero or NaN target excludes its pixel); pixel_weight: optional [1,H,W] or [H,W]
    plane of weights >= 0 (a value that is not > 0 excludes its pixel).  A pixel counts when its normal is valid (depth_normals),
    its target is and its weight is; the sum is divided by ALL pixels, as depth_l1 -- normal_count gives the number that counted,
    for renormalising.  One HIP pass and a one-workgroup reduction forward (double, fixed order), one gather pass backward that
    recomputes the normals (lr_normal_loss_forward / _backward).  Gradients flow to `depth` only."""
    return _NormalLoss.apply(depth, target_normals, camera, pixel_weight, weight)


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth_a, depth_b, camera, pixel_weight, weight):
        out, fields, keep = _loss_forward(depth_a, None, depth_b, camera, pixel_weight, weight, "normal_consistency")
        ctx.save_for_backward(*keep)
        ctx.fields, ctx.shapes = fields, (depth_a.shape, depth_b.shape)
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        a, b = ctx.saved_tensors[:2]
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        up = _weight(grad_out, a.device)
        f = dict(ctx.fields, upstream=up.data_ptr())
        ga = gb = None
        if need_a:
            ga = torch.empty_like(a)
            f["dL_ddepth"] = ga.data_ptr()
            if need_b:
                gb = torch.empty_like(b)
                f["dL_dtarget_depth"] = gb.data_ptr()
        elif need_b:                          # only the second depth: the term is symmetric, it takes the first one's place
            gb = torch.empty_like(b)
            f.update(depth=b.data_ptr(), target_depth=a.data_ptr(), dL_ddepth=gb.data_ptr())
        if need_a or need_b:
            _call(_lib.lib().lr_normal_loss_backward, "normal_consistency backward", a.device, **f)
        return (None if ga is None else ga.view(ctx.shapes[0]), None if gb is None else gb.view(ctx.shapes[1]), None, None, None)


def normal_consistency(depth_a, depth_b, camera, pixel_weight=None, weight=1.0):
    """normal_loss with the normals of a second depth map as the target: weight * sum of w_p (1 - n_a . n_b) / (H*W) over the
    pixels where both normals are valid -- e.g. the expected depth against the median depth (return_median=True).  Gradients go
    to both depths; a depth passed detached gets none, and nothing is computed for it.  (The median depth's gradient reaches the
    means only.)"""
    return _NormalConsistency.apply(depth_a, depth_b, camera, pixel_weight, weight)


def rendered_normal_consistency(rendered_normals, depth, camera, weight=1.0):
    """The normal consistency of 2DGS section 5 / RaDe-GS / PGSR between the RENDERED normal map N [3,H,W] (return_normals=True:
    the blend of the Gaussians' own normals, not normalised) and the normals n of the rendered depth:
    weight * sum over the valid pixels of (1 - N_p . n_p) / (H*W), n = depth_normals(depth, camera), valid = the pixels with a
    valid depth normal.  Composed from depth_normals and three torch ops; gradients go to both arguments -- through N to the
    rotations directly, which two depth maps (normal_consistency) reach only at second hand."""
    n = depth_normals(depth, camera)
    N = _normal_image(rendered_normals, "rendered_normals", "rendered_normal_consistency", n)
    valid = (n.detach() != 0).any(dim=0).sum()          # an invalid normal is (0,0,0): its dot product is an exact zero
    return (valid - (N * n).sum()) * (float(weight) / float(n.shape[-2] * n.shape[-1]))


def normal_count(depth, target, camera, pixel_weight=None):
    """The number of pixels that count in normal_loss (target [3,H,W]) or normal_consistency (target a depth map [1,H,W] or
    [H,W]) of these inputs: a 0-dim device tensor without a gradient, for renormalising (loss * H * W / count) and logging."""
    with torch.no_grad():
        as_normals = target.dim() == 3 and target.shape[0] == 3
        out, _, _ = _loss_forward(depth.detach(), target if as_normals else None, None if as_normals else target, camera,
                                  pixel_weight, 1.0, "normal_count")
        return out[1]


def normals_to_rgb(normals, uint8=False):
    """0.5 - 0.5 n: a normal map [3,H,W] (or [N,3,H,W]) as colours in [0, 1], a surface facing the camera (n = (0,0,-1)) in the
    usual light blue; invalid pixels (0,0,0) are mid grey.  uint8=True: the [H,W,3] bytes of video.frames_to_uint8 of it."""
    rgb = 0.5 - 0.5 * normals.detach()
    if uint8:
        from .video import frames_to_uint8
        return frames_to_uint8(rgb)
    return rgb
