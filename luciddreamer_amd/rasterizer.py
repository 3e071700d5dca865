"""Python operator of the MI355X rasterizer: same public API as the reference's
`depth_diff_gaussian_rasterization_min` package (RAST/depth_diff_gaussian_rasterization_min/__init__.py):

    GaussianRasterizationSettings   12-field NamedTuple, same names and order   (:158-170)
    GaussianRasterizer              nn.Module; forward(...) -> (color, radii, depth); markVisible (:172-221)
    rasterize_gaussians             functional entry                                (:21-42)

Beyond the reference: return_alpha=True (GaussianRasterizer.forward, rasterize_gaussians, rasterize_gaussians_raw) returns
(color, radii, depth, alpha) -- alpha (1, H, W) = 1 - T_final, the accumulated opacity, differentiable (lr_view_backward with dL_dalpha).
return_median=True (same three entry points) appends (median_depth, median_ids) to the outputs: median_depth (1, H, W) is the view-space
depth of the Gaussian at which the pixel's transmittance first falls below one half (0 where it never does), median_ids (H, W) int32
that Gaussian's row (-1 where there is none; not differentiable) -- lr_render_median, a pass behind the forward.  Unlike the expected
depth it never lies between a foreground and a background surface.  Its gradient reaches means3D / xyz only (the selection is a
constant; nothing flows to opacity, covariance or colour): a weaker signal than the expected depth's, enough for loss.depth_l1 /
loss.depth_pearson on the median depth.
return_distortion=True (same three entry points) appends distortion (1, H, W) LAST, behind alpha and the median pair: the depth distortion
of the pixel's blended layers (Mip-NeRF 360 / 2DGS / gsplat's `distloss`), D = sum_i w_i sum_{j<i} w_j (m_i - m_j)^2 with w_i the blend
weights and m_i the mapped depth of `distortion_map` -- "ndc" (default; ("ndc", near, far), 2DGS's far / (far - near) (1 - near / z) with
near = 0.2, far = 100) or "linear" (m = z) -- lr_render_distortion, a pass behind the forward.  Differentiable: a gradient reaching it runs
lr_distortion_backward behind the view's backward and reaches means3D / xyz, opacities, scales, rotations (cov3D) and means2D.
return_normals=True (same three entry points) appends normals (3, H, W) behind the median pair and in front of the distortion, which
stays the last output: the rendered normal map N = sum_i w_i n_i over the pixel's blended layers, n_i the Gaussian's view-space normal
-- its shortest axis (argmin of the scales as given, lowest index on ties: an isotropic Gaussian, as LucidDreamer's freshly
initialised ones, takes axis 0), rotated by the view matrix (x right, y down, z forward: normals.depth_normals' axes) and turned
towards the camera -- lr_render_normals, a pass behind the forward.  No background term, no normalisation: |N| <= alpha.  Needs
scales + rotations (ValueError with cov3D_precomp).  Differentiable: a gradient reaching it runs lr_render_normals_backward behind the
view's backward (and the distortion's) and reaches means3D / xyz, opacities, scales, rotations and means2D; the normal itself moves
the rotations only (the axis choice and the sign are constants of the view).
features=<(P, C) float32 tensor> (same three entry points) appends feature_map (C, H, W) behind the normals and in front of the
distortion, which stays the last output: F[c] = sum_i w_i features[i, c] over the pixel's blended layers (semantic or instance
logits, distilled 2D features, appearance codes; 1 <= C <= 256), used as given in both nodes -- lr_render_features, a pass behind the
forward, 16 channels per tile walk.  No background term, no normalisation.  Works with cov3D_precomp.  Differentiable: a gradient
reaching it runs lr_render_features_backward behind the view's backward (and the distortion's and the normals'), reaches means3D /
xyz, opacities, scales, rotations (cov3D) and means2D as the other passes' terms do, and `features` itself.  ValueError for a wrong
shape, dtype or row count, before any launch.
config.set_absgrad(True): the backward of a view attaches `means2D.absgrad` [P,3] (AbsGS; lr_view_backward with dL_dmean2D_abs) to the means2D
tensor the caller passed.

Error behaviour mirrored: plain `Exception` for bad SH/colour or scale/rotation/covariance
combinations (:192-196); with settings.debug the inputs of a failing call are dumped to
snapshot_fw.dump / snapshot_bw.dump before re-raising (:83-90, :133-140).
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C
from . import config


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _take_ticket():
    """The early-header request of a forward is ALWAYS withdrawn, also when the forward raised: a request left
    behind would make an unrelated later forward on this thread post a ticket nobody takes.  If the forward failed after the
    ticket was posted, a ticket of the copy-and-event kind is waited for once, which releases it (log tickets hold nothing)."""
    import sys
    ticket = _C.take_early_ticket()
    if sys.exc_info()[0] is not None and 0 <= ticket < (1 << 40):
        try:
            _C.header_poll(ticket, True)
        except Exception:
            pass
        return -1
    return ticket


def _forward(means3D, rs, capacity, run, node=False):
    """The forward of every entry point: run(capacity) under the overflow policy; returns (run's result, capacity used).
    capacity: config.capacity_for(means3D, rs), taken by the caller (rasterize_gaussians picks its route by it).
    node: run returns the compiled node's outputs (color, radii, depth, geom[, alpha]) with num_rendered in
    last_num_rendered(), else the binding's (num_rendered, color, depth, radii, geom, binning, img)."""
    verifying = config.verifying(capacity)
    ticket = -1
    if verifying:
        _C.request_early_header()
    try:
        out = run(capacity)
    finally:
        if verifying:
            ticket = _take_ticket()
    # policy "verify" (config.py): the whole forward is enqueued; wait for the copy of the header the library posted after the
    # scan, and if the view needs more instances than its buffer holds render it again in exact mode -- what is returned is
    # always a complete image (a first autograd node is simply dropped)
    if verifying and config.verify(means3D, rs, ticket):
        capacity = 0
        out = run(0)
    num_rendered, geom = (_C.last_num_rendered(), out[3]) if node else (out[0], out[4])
    config.note_forward(means3D, rs, num_rendered, geom, capacity)
    return out, capacity


def _fusable_grad(t, device):
    """t.grad if a backward kernel may add into it in place (config.set_fused_grad_accumulation), else None: t a non-empty
    leaf that requires grad, its .grad contiguous float32 on `device` and 16-byte aligned (the kernels accumulate with
    16-byte accesses).  csrc/torch_ext.cpp fusable_grad is the same rule."""
    g = t.grad if (t.is_leaf and t.requires_grad and t.numel() != 0) else None
    if g is not None and g.is_contiguous() and g.dtype == torch.float32 and g.device == device and g.data_ptr() % 16 == 0:
        return g
    return None


def _snapshot(args, path):
    torch.save(tuple(a.detach().cpu().clone() if isinstance(a, torch.Tensor) else a for a in args), path)


def _median_outputs(ctx, P, rs, geom, binning, img, capacity):
    """(median_depth, median_ids) of the forward whose buffers are given -- after an overflow re-render the re-render's, as alpha's --
    and what the backward of a node needs of them: the ids (not differentiable, so keeping them on ctx is no reference cycle)."""
    median_depth, median_ids = _C.render_median(geom, binning, img, P, rs.image_height, rs.image_width, binning_capacity=capacity)
    ctx.mark_non_differentiable(median_ids)
    ctx.median_ids = median_ids
    return median_depth, median_ids


def _distortion_outputs(ctx, P, rs, geom, binning, img, capacity, distortion_map):
    """(distortion,) of the forward whose buffers are given, as _median_outputs; the backward needs the moments image, the value
    (detached: the output itself on ctx would be a reference cycle) and the mapping."""
    distortion, moments = _C.render_distortion(geom, binning, img, P, rs.image_height, rs.image_width,
                                               distortion_map=distortion_map, binning_capacity=capacity)
    ctx.distortion = (distortion.detach(), moments, distortion_map)
    return (distortion,)


def _normals_outputs(ctx, rs, radii, geom, binning, img, capacity, inputs):
    """(normals,) of the forward whose buffers are given, as _distortion_outputs; the backward needs the value (detached) and the
    per-Gaussian normals.  inputs: means3D, scales, rotations, cov3D_precomp[, raw] of the node."""
    normals, gauss_normals = _C.render_normals(geom, binning, img, radii, rs, binning_capacity=capacity, **inputs)
    ctx.normals = (normals.detach(), gauss_normals)
    return (normals,)


def _features_outputs(ctx, rs, geom, binning, img, capacity, features):
    """(feature_map,) of the forward whose buffers are given, as _normals_outputs; the backward needs the value (detached) and the
    features as they were rendered (detached: the gradient goes to the node's input)."""
    value = _C.render_features(geom, binning, img, features, rs, binning_capacity=capacity)
    ctx.features = (value.detach(), features.detach())
    return (value,)


def _more_grads(ctx, grad_more):
    """(grad_alpha, grad_median, grad_distortion, grad_normals, grad_features) from the gradients behind (color, radii, depth):
    [alpha], [median_depth, median_ids], [normals], [feature_map], [distortion]."""
    tail = 1 if ctx.distortion is not None else 0
    ftr = 1 if ctx.features is not None else 0
    nrm = 1 if ctx.normals is not None else 0
    grad_alpha = grad_more[0] if ctx.return_alpha else None
    grad_median = grad_more[-2 - tail - ftr - nrm] if ctx.median_ids is not None else None
    grad_normals = grad_more[-1 - tail - ftr] if nrm else None
    grad_features = grad_more[-1 - tail] if ftr else None
    grad_distortion = grad_more[-1] if tail else None
    return grad_alpha, grad_median, grad_distortion, grad_normals, grad_features


def _median_backward(ctx, grad_median, target, radii, geom, binning, img):
    """The median depth's term of dL/dmeans3D (lr_median_backward), added behind the view's backward on the same stream into
    `target`: the tensor that backward returned, or, where it accumulated into the leaf's .grad in place (returned None), that
    .grad -- the same additions in the same order either way."""
    _C.median_backward(geom, binning, img, radii, ctx.median_ids, grad_median, ctx.raster_settings.viewmatrix,
                       binning_capacity=ctx.binning_capacity, accumulate_into=target)


def _side_backward(call, names, returned, fused, plus_zero):
    """The term of one pass behind the forward in every geometric gradient, added behind the view's backward on the same stream: per
    tensor into what that backward returned, or, where it accumulated into the leaf's .grad in place (returned None), into that
    .grad -- the same additions in the same order either way.  returned / fused: {name: tensor or None} under the names of
    _C.distortion_backward; names: those the pass has a gradient for; call(targets): its _C.*_backward with accumulate_into.
    plus_zero: the tensors the view's backward RETURNED (written, then added to) end with +0 for their zero entries, as the same
    sums have when they are accumulated into a zeroed .grad -- a Gaussian the view visited and no pixel blended is written as
    -0 by the per-Gaussian kernel, and -0 + -0 stays -0 where +0 + -0 + -0 is +0: with it the fused and the unfused route give
    the same bits.  One multi-tensor launch; not for the armed optimizer step, whose rows are read through the view's mask.
    Returns (`returned` with the term: an input neither of the two covers gets the term alone, the call's dict)."""
    targets = {k: (returned[k] if returned[k] is not None else fused.get(k)) for k in names}
    out = call(targets)
    written = [returned[k] for k in names if returned[k] is not None]
    if plus_zero and written:
        torch._foreach_add_(written, 0.0)
    return dict(returned, **{k: (returned[k] if (returned[k] is not None or fused.get(k) is not None) else out[k]) for k in names}), out


def _distortion_backward(ctx, grad_distortion, returned, fused, geom, binning, img, **inputs):
    """The distortion's term (lr_distortion_backward): the one pass whose term is added without the +0 rule."""
    value, moments, distortion_map = ctx.distortion
    call = lambda targets: _C.distortion_backward(geom, binning, img, grad_distortion, value, moments, ctx.raster_settings,
                                                  distortion_map=distortion_map, binning_capacity=ctx.binning_capacity,
                                                  accumulate_into=targets, **inputs)
    return _side_backward(call, tuple(returned), returned, fused, False)[0]


def _normals_backward(ctx, grad_normals, returned, fused, radii, geom, binning, img, plus_zero=True, **inputs):
    """The rendered normal map's term (lr_render_normals_backward), behind the distortion's.  cov3D never takes part: there is no
    normal without scales + rotations."""
    value, gauss_normals = ctx.normals
    call = lambda targets: _C.render_normals_backward(geom, binning, img, grad_normals, value, gauss_normals, radii,
                                                      ctx.raster_settings, binning_capacity=ctx.binning_capacity,
                                                      accumulate_into=targets, **inputs)
    return _side_backward(call, ("means2D", "opacity", "means3D", "scales", "rotations"), returned, fused, plus_zero)[0]


def _features_backward(ctx, grad_features, returned, fused, radii, geom, binning, img, plus_zero=True, **inputs):
    """The feature map's term and dL/dfeatures (lr_render_features_backward), behind the normals'; cov3D takes part.  Returns
    (`returned` with the term, dL/dfeatures or None where it was accumulated into the leaf's .grad)."""
    value, features = ctx.features
    call = lambda targets: _C.render_features_backward(geom, binning, img, grad_features, value, features, radii, ctx.raster_settings,
                                                       slots=ctx.num_rendered, binning_capacity=ctx.binning_capacity,
                                                       accumulate_into=dict(targets, features=fused.get("features")), **inputs)
    returned, out = _side_backward(call, tuple(returned), returned, fused, plus_zero)
    return returned, (None if fused.get("features") is not None else out["features"])


def _forward_tail(ctx, out, P, rs, geom, binning, img, capacity, return_alpha, return_median, return_distortion, distortion_map,
                  return_normals=False, normal_inputs=None, features=None):
    """The end of both nodes' forward: `out` = (color, radii, depth) gains alpha, (median_depth, median_ids), normals, feature_map,
    distortion, in that order, from the state of the forward whose buffers are given (after a re-render, the re-render's), and ctx
    what they need."""
    ctx.return_alpha = bool(return_alpha)
    ctx.median_ids = None
    ctx.distortion = None
    ctx.normals = None
    ctx.features = None
    if not return_alpha and not return_median and not return_distortion and not return_normals and features is None:
        return out
    # the backward needs the image state's final T only -- the alpha tensor itself is not kept (as depth_image)
    ctx.set_materialize_grads(False)            # an unused alpha / median / distortion output arrives as None: the default kernels
    if return_alpha:
        out += (_C.render_alpha(img, rs.image_height, rs.image_width),)
    if return_median:
        out += _median_outputs(ctx, P, rs, geom, binning, img, capacity)
    if return_normals:
        out += _normals_outputs(ctx, rs, out[1], geom, binning, img, capacity, normal_inputs)
    if features is not None:
        out += _features_outputs(ctx, rs, geom, binning, img, capacity, features)
    if return_distortion:
        out += _distortion_outputs(ctx, P, rs, geom, binning, img, capacity, distortion_map)
    return out


def _backward_extras(ctx, grad_median, grad_distortion, grad_normals, returned, fused, radii, geom, binning, img, armed=False,
                     grad_features=None, **inputs):
    """The median depth's term, then the distortion's, then the rendered normals', then the feature map's, added behind the view's
    backward.  returned / fused: {name: tensor or None} of what that backward returned / of the leaves' .grad it accumulated into,
    under _C.distortion_backward's names, as `inputs` (fused["features"]: the features' .grad).  Returns (returned, dL/dfeatures --
    None without grad_features, and where it was accumulated into the leaf's .grad)."""
    fused = fused or {}
    if grad_median is not None:
        m3 = returned["means3D"]
        _median_backward(ctx, grad_median, m3 if m3 is not None else fused.get("means3D"), radii, geom, binning, img)
    if grad_distortion is not None:
        returned = _distortion_backward(ctx, grad_distortion, returned, fused, geom, binning, img, **inputs)
    if grad_normals is not None:
        returned = _normals_backward(ctx, grad_normals, returned, fused, radii, geom, binning, img, plus_zero=not armed, **inputs)
    grad_of_features = None
    if grad_features is not None:
        returned, grad_of_features = _features_backward(ctx, grad_features, returned, fused, radii, geom, binning, img,
                                                        plus_zero=not armed, **inputs)
    return returned, grad_of_features


_RAW_NAMES = dict(xyz="means3D", scaling="scales", rotation="rotations")     # the raw node's names -> _C.distortion_backward's
_from_raw_names = lambda d: {_RAW_NAMES.get(k, k): v for k, v in (d or {}).items()}


class _RasterizeGaussians(torch.autograd.Function):
    """forward/backward wiring of RAST/.../__init__.py:44-156."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, return_alpha=False, return_median=False, return_distortion=False, distortion_map="ndc",
                return_normals=False, features=None):
        rs = raster_settings
        if return_normals:                              # before any launch
            _C.require_scale_rot("return_normals", scales, rotations, cov3Ds_precomp)
        if features is not None:
            _C.require_features("features", features, means3D.shape[0])
        args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh,
                rs.sh_degree, rs.campos, rs.prefiltered, rs.debug)
        capacity = config.capacity_for(means3D, rs)
        ctx.antialiasing = config.antialiasing()        # as this forward finds it: backward checks (config.set_antialiasing)
        ctx.absgrad_to = means2D if config.absgrad() else None      # config.set_absgrad as it is at this forward
        try:
            (num_rendered, color, depth, radii, geom, binning, img), capacity = _forward(
                means3D, rs, capacity, lambda cap: _C.rasterize_gaussians(*args, binning_capacity=cap))
        except Exception:
            if rs.debug:
                _snapshot(args, "snapshot_fw.dump")
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
            raise
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        ctx.binning_capacity = capacity
        # leaf inputs whose .grad already exists can be accumulated into in place by the backward kernel
        ctx.leaf_inputs = dict(means3D=means3D, means2D=means2D, sh=sh, colors=colors_precomp, opacity=opacities,
                               scales=scales, rotations=rotations, cov3D=cov3Ds_precomp, features=features) \
            if config.fused_grad_accumulation() else None
        # config.set_depth_gradient as it is at this forward: the depth image is kept for a depth-mode backward
        # (detached: the output itself on ctx would be a reference cycle through its grad_fn, freed only by the cyclic GC)
        ctx.depth_image = depth.detach() if config.depth_gradient() else None
        if ctx.depth_image is not None:
            ctx.set_materialize_grads(False)        # an unused depth output arrives as None: the default kernels
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning, img)
        return _forward_tail(ctx, (color, radii, depth), means3D.shape[0], rs, geom, binning, img, capacity, return_alpha,
                             return_median, return_distortion, distortion_map, return_normals,
                             dict(means3D=means3D, scales=scales, rotations=rotations, cov3D_precomp=cov3Ds_precomp), features)

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_depth, *grad_more):
        grad_alpha, grad_median, grad_distortion, grad_normals, grad_features = _more_grads(ctx, grad_more)
        config.require_antialiasing(ctx.antialiasing)   # before anything is launched or written
        rs = ctx.raster_settings
        colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning, img = ctx.saved_tensors
        if grad_out_color is None:
            grad_out_color = torch.zeros((3, rs.image_height, rs.image_width), dtype=torch.float32, device=means3D.device)
        args = (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, grad_depth, sh, rs.sh_degree,
                rs.campos, geom, ctx.num_rendered, binning, img, rs.debug)
        accumulate_into = None
        if ctx.leaf_inputs is not None:                 # an input without a fusable .grad (None): the dense path
            accumulate_into = {name: _fusable_grad(t, means3D.device) for name, t in ctx.leaf_inputs.items() if t is not None}
        try:
            # the binding picks the mode: depth mode needs the kept depth image (switch on at the forward) and grad_depth
            g = _C.rasterize_gaussians_backward(
                *args, binning_capacity=ctx.binning_capacity, accumulate_into=accumulate_into, skip_unused=True,
                depth_image=ctx.depth_image, dL_dout_alpha=grad_alpha, absgrad=ctx.absgrad_to is not None)
            (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
             grad_scales, grad_rotations) = g[:8]
            if ctx.absgrad_to is not None:              # gsplat's convention; replaced at every backward
                ctx.absgrad_to.absgrad = g[8]
            d, grad_of_features = _backward_extras(
                ctx, grad_median, grad_distortion, grad_normals,
                dict(means2D=grad_means2D, opacity=grad_opacities, means3D=grad_means3D, scales=grad_scales,
                     rotations=grad_rotations, cov3D=grad_cov3Ds_precomp),
                accumulate_into, radii, geom, binning, img, grad_features=grad_features, means3D=means3D, scales=scales,
                rotations=rotations, cov3D_precomp=cov3Ds_precomp)
            grad_means2D, grad_opacities, grad_means3D = d["means2D"], d["opacity"], d["means3D"]
            grad_scales, grad_rotations, grad_cov3Ds_precomp = d["scales"], d["rotations"], d["cov3D"]
        except Exception:
            if rs.debug:
                _snapshot(args, "snapshot_bw.dump")
                print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
            raise
        # order of the forward inputs (RAST/.../__init__.py:144-154); gradients of absent inputs are None-able
        return (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales, grad_rotations,
                grad_cov3Ds_precomp, None, None, None, None, None, None, grad_of_features)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, return_alpha=False, return_median=False, return_distortion=False, distortion_map="ndc",
                        return_normals=False, features=None):
    """The operator.  Its autograd node is compiled (csrc/torch_ext.cpp RasterizeFn: forward and backward run without the
    interpreter -- the Python node below cost more host time per 1080p view than the GPU needs for it); with settings.debug
    the Python node runs instead, because it is the one that writes the reference's snapshot_fw.dump / snapshot_bw.dump.
    return_alpha: (color, radii, depth, alpha) -- alpha = 1 - T_final (1, H, W), differentiable; a gradient reaching it runs the
    alpha-mode backward (lr_view_backward with dL_dalpha), an unused alpha output the default one.
    return_median: the outputs gain (median_depth, median_ids) at their end (module docstring).  Such a call always runs the
    Python node, which holds the forward's geom, binning and image buffers in hand as debug does -- never the compiled node or
    the one-call rasterize_view_step route: the interpreter's share of a view (the node's forward and backward, plus two ctypes
    calls and two small launches) is paid per call, which at 1080p is more host time than the GPU needs for the view.  Unused
    median outputs leave the backward exactly as it is without them; a gradient reaching median_depth adds its term to the
    gradient of means3D, with config.set_fused_grad_accumulation on or off.
    return_distortion: the outputs gain distortion (1, H, W) as their LAST entry (module docstring), for the mapped depth of
    distortion_map.  As return_median it always runs the Python node; an unused distortion output leaves the backward exactly as it
    is, a gradient reaching it runs lr_distortion_backward behind the view's backward, fused accumulation on or off.
    return_normals: the outputs gain normals (3, H, W), the rendered normal map (module docstring), behind the median pair and in
    front of the distortion.  Needs scales + rotations (ValueError otherwise, before any launch).  As its siblings it always runs
    the Python node; an unused normals output leaves the backward exactly as it is, a gradient reaching it runs
    lr_render_normals_backward behind the view's backward (and the distortion's), fused accumulation on or off.
    features: a (P, C) float32 tensor; the outputs gain feature_map (C, H, W) (module docstring) behind the normals and in front
    of the distortion.  ValueError for a wrong shape, dtype or row count, before any launch.  As its siblings it always runs the
    Python node; an unused feature output leaves the backward exactly as it is and launches nothing, a gradient reaching it runs
    lr_render_features_backward behind the view's backward (and the distortion's and the normals'), fused accumulation on or off,
    and `features` receives its gradient."""
    rs = raster_settings
    if rs.debug or return_median or return_distortion or return_normals or features is not None:
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                         cov3Ds_precomp, rs, bool(return_alpha), bool(return_median), bool(return_distortion),
                                         distortion_map, bool(return_normals), features)
    capacity = config.capacity_for(means3D, rs)
    fused = config.fused_grad_accumulation()
    offered = config.offered_grad_output()
    absgrad = config.absgrad()
    # (an alpha-requesting call never takes the direct route: its backward would not see a gradient of alpha)
    if offered is not None and fused and not return_alpha and not config.verifying(capacity):
        # the caller already holds dL/dcolor (parallel.ViewStreams.run_view): forward and backward in ONE call of the binding,
        # gradients added into the leaves' .grad by the kernels, no autograd node (csrc/torch_ext.cpp rasterize_view_step).
        # An input that is not a leaf with a suitable .grad -> empty result -> the autograd path below, offer untouched.
        # An offered dL/ddepth selects the depth-mode backward (fed with this forward's own depth image).
        out = _C.rasterize_view_step(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs.bg,
                                     rs.viewmatrix, rs.projmatrix, rs.campos, rs.scale_modifier, rs.tanfovx, rs.tanfovy,
                                     rs.image_height, rs.image_width, rs.sh_degree, rs.prefiltered, capacity, offered,
                                     config.offered_grad_depth(), absgrad)
        if out:
            color, radii, depth, geom = out[:4]
            if absgrad:                                 # the backward has run: as the nodes do at theirs
                means2D.absgrad = out[4]
            config.mark_grad_output_taken((color, depth))
            config.note_forward(means3D, rs, _C.last_num_rendered(), geom, capacity)
            return color, radii, depth

    def run(cap):
        return _C.rasterize_autograd(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs.bg,
                                     rs.viewmatrix, rs.projmatrix, rs.campos, rs.scale_modifier, rs.tanfovx, rs.tanfovy,
                                     rs.image_height, rs.image_width, rs.sh_degree, rs.prefiltered, cap, fused,
                                     config.depth_gradient(), bool(return_alpha), absgrad)
    out, _ = _forward(means3D, rs, capacity, run, node=True)
    if return_alpha:
        return out[0], out[1], out[2], out[4]
    return out[0], out[1], out[2]


class _RasterizeGaussiansRaw(torch.autograd.Function):
    """Autograd op over the STORED GaussianModel tensors: one forward and one backward call replace
    exp / normalize / sigmoid / cat and their autograd nodes (R/scene/gaussian_model.py:97-117)."""

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, raster_settings, return_alpha=False,
                return_median=False, return_distortion=False, distortion_map="ndc", return_normals=False, features=None):
        rs = raster_settings
        if features is not None:                        # before any launch
            _C.require_features("features", features, xyz.shape[0])
        ctx.antialiasing = config.antialiasing()        # as _RasterizeGaussians
        ctx.absgrad_to = means2D if config.absgrad() else None

        def run(cap):
            return _C.rasterize_gaussians_raw(
                rs.bg, xyz, features_dc, features_rest, opacity, scaling, rotation, rs.scale_modifier, rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.sh_degree, rs.campos, rs.debug,
                binning_capacity=cap)
        (num_rendered, color, depth, radii, geom, binning, img), capacity = _forward(xyz, rs, config.capacity_for(xyz, rs), run)
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        ctx.binning_capacity = capacity
        ctx.leaf_inputs = dict(xyz=xyz, means2D=means2D, features_dc=features_dc, features_rest=features_rest,
                               opacity=opacity, scaling=scaling, rotation=rotation, features=features) \
            if config.fused_grad_accumulation() else None
        ctx.depth_image = depth.detach() if config.depth_gradient() else None       # as _RasterizeGaussians
        if ctx.depth_image is not None:
            ctx.set_materialize_grads(False)
        ctx.save_for_backward(xyz, features_dc, features_rest, opacity, scaling, rotation, radii, geom, binning, img)
        return _forward_tail(ctx, (color, radii, depth), xyz.shape[0], rs, geom, binning, img, capacity, return_alpha,
                             return_median, return_distortion, distortion_map, return_normals,
                             dict(means3D=xyz, scales=scaling, rotations=rotation, raw=True), features)

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_depth, *grad_more):
        grad_alpha, grad_median, grad_distortion, grad_normals, grad_features = _more_grads(ctx, grad_more)
        config.require_antialiasing(ctx.antialiasing)   # before anything is launched or written
        rs = ctx.raster_settings
        xyz, features_dc, features_rest, opacity, scaling, rotation, radii, geom, binning, img = ctx.saved_tensors
        if grad_out_color is None:
            grad_out_color = torch.zeros((3, rs.image_height, rs.image_width), dtype=torch.float32, device=xyz.device)
        # what arrived, as _RasterizeGaussians.backward: the binding picks the depth / alpha mode from it
        modes = dict(dL_dout_depth=grad_depth, depth_image=ctx.depth_image, dL_dout_alpha=grad_alpha,
                     absgrad=ctx.absgrad_to is not None)
        accumulate_into = None
        if ctx.leaf_inputs is not None:
            li = ctx.leaf_inputs
            accumulate_into = {k: _fusable_grad(li[k], xyz.device) for k in ("xyz", "means2D", "opacity", "scaling", "rotation")}
            g_dc, g_rest = _fusable_grad(li["features_dc"], xyz.device), _fusable_grad(li["features_rest"], xyz.device)
            if g_dc is not None and (g_rest is not None or features_rest.numel() == 0):
                accumulate_into["features"] = (g_dc, g_rest)
        # the feature table's .grad (the raw backward's "features" are the SH pair above)
        fused_table = _fusable_grad(ctx.leaf_inputs["features"], xyz.device) \
            if (ctx.leaf_inputs is not None and ctx.leaf_inputs["features"] is not None) else None
        def extras(g, fused, armed=False):
            # the median's and the distortion's terms on the result g of the raw backward, under the activated node's names
            returned = _from_raw_names(dict(means2D=g[0], xyz=g[1], opacity=g[4], scaling=g[5], rotation=g[6]))
            fused = {k: v for k, v in _from_raw_names(fused).items() if k != "features"}
            fused["features"] = fused_table
            return _backward_extras(ctx, grad_median, grad_distortion, grad_normals, returned, fused, radii, geom,
                                    binning, img, armed=armed, grad_features=grad_features,
                                    means3D=xyz, opacities=opacity, scales=scaling, rotations=rotation, raw=True)

        # an armed FusedAdam over exactly these six tensors (optim.FusedAdam.arm_fused_backward): the gradients go to tensors
        # autograd never sees -- visited rows only, nothing zero-filled -- and the optimizer's masked step
        # (lr_adam_step_masked: the view's own visibility is the mask) is launched right behind the backward's kernels;
        # optimizer.step() later only checks the iteration.  param.grad stays None.
        from . import optim
        opt = optim.take_armed((xyz, features_dc, features_rest, opacity, scaling, rotation)) \
            if (optim._armed is not None and not rs.debug and all(ctx.needs_input_grad[k] for k in (0, 2, 4, 5, 6))) else None
        if opt is not None:
            g = _C.rasterize_gaussians_raw_backward(
                rs.bg, xyz, radii, features_dc, features_rest, opacity, scaling, rotation, rs.scale_modifier, rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, rs.sh_degree, rs.campos, geom, ctx.num_rendered,
                binning, img, False, binning_capacity=ctx.binning_capacity, no_zero_fill=True, **modes)
            if ctx.absgrad_to is not None:              # written in full also here (zero-filled like means2D): not part of the step
                ctx.absgrad_to.absgrad = g[7]
            # the rows the extras add to are rows the view visited; before the step reads them
            _, g_table = extras(g, None, armed=True)
            opt.apply_armed_step(geom, [xyz, features_dc, features_rest, opacity, scaling, rotation], list(g[1:7]))
            return None, g[0], None, None, None, None, None, None, None, None, None, None, None, g_table
        g = _C.rasterize_gaussians_raw_backward(
            rs.bg, xyz, radii, features_dc, features_rest, opacity, scaling, rotation, rs.scale_modifier, rs.viewmatrix,
            rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, rs.sh_degree, rs.campos, geom, ctx.num_rendered,
            binning, img, rs.debug, binning_capacity=ctx.binning_capacity, accumulate_into=accumulate_into, **modes)
        if ctx.absgrad_to is not None:
            ctx.absgrad_to.absgrad = g[7]
        g_dc, g_rest = g[2], g[3]
        d, g_table = extras(g, accumulate_into)
        g_means2D, g_op, g_xyz, g_sc, g_rot = d["means2D"], d["opacity"], d["means3D"], d["scales"], d["rotations"]
        return g_xyz, g_means2D, g_dc, g_rest, g_op, g_sc, g_rot, None, None, None, None, None, None, g_table


def rasterize_gaussians_raw(xyz, means2D, features_dc, features_rest, opacity, scaling, rotation, raster_settings,
                            return_alpha=False, return_median=False, return_distortion=False, distortion_map="ndc",
                            return_normals=False, features=None):
    """(color, radii, depth) from the stored GaussianModel parameters (pre-activation), see _RasterizeGaussiansRaw;
    return_alpha: (color, radii, depth, alpha) as rasterize_gaussians; return_median: (median_depth, median_ids) behind them, as
    rasterize_gaussians (this entry point always runs its Python node); the median depth's gradient reaches xyz;
    return_distortion / distortion_map: distortion last, as rasterize_gaussians; its gradient reaches xyz, opacity, scaling and
    rotation; return_normals: normals (3, H, W) behind the median pair, in front of the distortion, as rasterize_gaussians (the
    axis is the argmin of the stored log-scales, the quaternion is normalised as the kernels normalise it); features: a (P, C)
    float32 tensor, feature_map (C, H, W) behind the normals and in front of the distortion, as rasterize_gaussians (used as
    given: the table has no activation)."""
    return _RasterizeGaussiansRaw.apply(xyz, means2D, features_dc, features_rest, opacity, scaling, rotation,
                                        raster_settings, bool(return_alpha), bool(return_median), bool(return_distortion),
                                        distortion_map, bool(return_normals), features)


_EMPTY = torch.Tensor([])           # never written: one instance serves every call (three constructions per call were ~6 us)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        """Boolean mask of points in front of the near plane (view z > 0.2)."""
        with torch.no_grad():
            rs = self.raster_settings
            return _C.mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, return_alpha=False, return_median=False, return_distortion=False, distortion_map="ndc",
                return_normals=False, features=None):
        """(color, radii, depth), or with return_alpha=True (color, radii, depth, alpha): alpha (1, H, W) = 1 - T_final; with
        return_median=True the outputs gain (median_depth, median_ids) at their end, with return_distortion=True the distortion
        (1, H, W) of distortion_map's mapped depth behind those, and with return_normals=True the rendered normal map (3, H, W)
        between the median pair and the distortion (rasterize_gaussians; ValueError with cov3D_precomp), and with
        features=<(P, C) float32 tensor> the feature map (C, H, W) behind the normals, in front of the distortion."""
        rs = self.raster_settings
        if (shs is None) == (colors_precomp is None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        scale_rot_given = scales is not None or rotations is not None
        scale_rot_complete = scales is not None and rotations is not None
        if (not scale_rot_complete and cov3D_precomp is None) or (scale_rot_given and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')

        empty = _EMPTY                  # the reference's placeholder for an absent optional input (`torch.Tensor([])`, :198-208)
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        if return_alpha or return_median or return_distortion or return_normals or features is not None:
            return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                       cov3D_precomp, rs, return_alpha=return_alpha, return_median=return_median,
                                       return_distortion=return_distortion, distortion_map=distortion_map,
                                       return_normals=return_normals, features=features)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, rs)
