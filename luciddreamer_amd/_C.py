"""Drop-in replacement of the reference's pybind11 module `depth_diff_gaussian_rasterization_min._C`.

Same three functions, same positional arguments, same return tuples:
    rasterize_gaussians           RAST/rasterize_points.h:18-38,  RAST/rasterize_points.cu:35-117
    rasterize_gaussians_backward  RAST/rasterize_points.h:40-63,  RAST/rasterize_points.cu:119-200
    mark_visible                  RAST/rasterize_points.h:65-68,  RAST/rasterize_points.cu:202-221
Tensors are torch tensors on a HIP device; the work is done by liblucid_raster.so through its C-ABI
(include/lucid_raster.h) on the CURRENT torch stream.  The marshalling (tensor checks, output and scratch
allocation, pointers, stream) is the compiled module `luciddreamer_amd._C_ext` (csrc/torch_ext.cpp, built in-tree by
`python -m luciddreamer_amd.build`); this file only adapts keyword conveniences to its positional interface.
There is no fallback: a missing extension raises on import.

Beyond the reference's contract (all optional, keyword-only):
    binning_capacity : > 0 runs lr_forward in async mode (no host sync; see lucid_raster.h)
    dL_dout_alpha    : the gradient of the alpha output (render_alpha), on both backward entry points
    absgrad          : absgrad mode (lr_view_backward with dL_dmean2D_abs), on both backward entry points
"""
try:
    from . import _C_ext
except ImportError as e:                                        # pragma: no cover - build problem, not a code path
    raise ImportError(
        "luciddreamer_amd: the compiled binding luciddreamer_amd/_C_ext*.so is missing or does not load "
        f"({e}); build it with `python -m luciddreamer_amd.build` (needs lib/liblucid_raster.so). "
        "There is no CPU / pure-Python fallback.") from e

import torch

from . import _lib as _lib_check
_lib_check.assert_single_copy()                                 # the binding and ctypes must be on ONE build of the library

NUM_CHANNELS = 3
# order of rasterize_gaussians_backward's result tuple (RAST/rasterize_points.cu:199) = order of `accumulate`
GRAD_ORDER = ("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations")
ACC_BITS = {"means2D": 0, "opacity": 2, "colors": 3, "means3D": 4, "cov3D": 5, "sh": 6, "scales": 7, "rotations": 8}
RAW_GRAD_ORDER = ("means2D", "xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
RAW_ACC_BITS = {"means2D": 0, "opacity": 2, "xyz": 4, "features": 6, "scaling": 7, "rotation": 8}
_NONE8 = []


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                        prefiltered, debug, *, binning_capacity=0):
    return _C_ext.rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                                      viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree,
                                      campos, prefiltered, debug, binning_capacity)


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                 dL_dout_depth, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                                 debug, *, binning_capacity=0, accumulate_into=None, skip_unused=False, depth_image=None,
                                 dL_dout_alpha=None, absgrad=False):
    """accumulate_into (optional): {name: tensor} with names among ACC_BITS; the gradient of that input is
    ADDED in place into the given contiguous float32 tensor (rows of culled Gaussians untouched) and the
    corresponding slot of the returned tuple is None.
    skip_unused: do not materialise gradients of inputs that are absent (dL_dcolors when SHs are used, dL_dcov3D /
    dL_dscales / dL_drotations for the representation not in use); their slots are None.  The reference always
    returns all eight tensors, so the default keeps that.
    depth_image (optional): the forward's depth output -- depth mode: dL_dout_depth is honoured.  Without it dL_dout_depth
    is ignored, as in the reference.
    dL_dout_alpha (optional, (1, H, W)): the gradient of the alpha output (render_alpha) as well, alone or together with depth
    mode.  Every mode, the default included, is one call of lr_view_backward with NULL for what is absent.
    absgrad: lr_view_backward with dL_dmean2D_abs as well; the result gains a ninth entry, dL_dmean2D_abs [P,3] (always a new tensor)."""
    acc = _NONE8 if not accumulate_into else [accumulate_into.get(k) for k in GRAD_ORDER]
    return tuple(_C_ext.rasterize_gaussians_backward(
        background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
        tan_fovx, tan_fovy, dL_dout_color, dL_dout_depth, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
        debug, binning_capacity, acc, skip_unused, depth_image=depth_image, dL_dout_alpha=dL_dout_alpha, absgrad=bool(absgrad)))


def rasterize_gaussians_raw(background, xyz, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw,
                            scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width,
                            degree, campos, debug, *, binning_capacity=0):
    """Forward on the STORED GaussianModel tensors (lr_view_forward with raw = 1): exp / normalize / sigmoid and
    the features_dc|features_rest split are handled inside the kernels.  Returns the tuple of rasterize_gaussians."""
    if opacity_raw is None:
        raise RuntimeError("rasterize_gaussians_raw: raw mode needs features_dc, features_rest (M > 1), opacity, "
                           "scaling and rotation")
    return _C_ext.rasterize_gaussians_raw(background, xyz, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw,
                                          scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height,
                                          image_width, degree, campos, debug, binning_capacity)


def rasterize_gaussians_raw_backward(background, xyz, radii, features_dc, features_rest, opacity_raw, scaling_raw,
                                     rotation_raw, scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                                     dL_dout_color, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, *,
                                     binning_capacity=0, accumulate_into=None, no_zero_fill=False, dL_dout_depth=None,
                                     depth_image=None, dL_dout_alpha=None, absgrad=False):
    """Gradients w.r.t. the stored tensors: (means2D, xyz, features_dc, features_rest, opacity, scaling, rotation).
    accumulate_into: {"means2D","xyz","opacity","scaling","rotation": tensor, "features": (dc_grad, rest_grad)} adds
    in place (slot returned as None).
    dL_dout_depth + depth_image (the forward's depth output): depth mode.
    dL_dout_alpha: the gradient of the alpha output as well.  Every mode is one call of lr_view_backward with raw = 1.
    absgrad: dL_dmean2D_abs given as well; the result gains an eighth entry, dL_dmean2D_abs [P,3]."""
    acc = _NONE8
    if accumulate_into:
        f = accumulate_into.get("features") or (None, None)
        acc = [accumulate_into.get("means2D"), accumulate_into.get("xyz"), f[0], f[1], accumulate_into.get("opacity"),
               accumulate_into.get("scaling"), accumulate_into.get("rotation")]
    return tuple(_C_ext.rasterize_gaussians_raw_backward(
        background, xyz, radii, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw, scale_modifier, viewmatrix,
        projmatrix, tan_fovx, tan_fovy, dL_dout_color, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug,
        binning_capacity, acc, bool(no_zero_fill), dL_dout_depth=dL_dout_depth, depth_image=depth_image,
        dL_dout_alpha=dL_dout_alpha, absgrad=bool(absgrad)))


# one Adam step whose gradients are valid only in the rows of the Gaussians one view visited (lr_adam_step_masked)
adam_step_masked = _C_ext.adam_step_masked
mark_visible = _C_ext.mark_visible
check = _C_ext.check
# the operator with its autograd node compiled (csrc/torch_ext.cpp RasterizeFn); returns (color, radii, depth, geom), the
# call's num_rendered is read with last_num_rendered()
rasterize_autograd = _C_ext.rasterize_autograd
# the alpha output 1 - T_final (1, H, W) of a forward, from its image buffer (lr_render_alpha); no autograd.  (With alpha=True
# rasterize_autograd returns it as a fifth, differentiable output.)
render_alpha = _C_ext.render_alpha


def _forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev, P=None, W=None, H=None):
    """The fields every argument struct of a pass behind a finished forward shares: its three buffers, the capacity it ran under, the
    current stream of `dev`, and (where the struct has no lr_view of its own) P, width, height."""
    import torch
    _buffers_on(dev, geomBuffer, binningBuffer, imageBuffer)
    f = dict(geom_buffer=geomBuffer.data_ptr(), binning_buffer=binningBuffer.data_ptr(), image_buffer=imageBuffer.data_ptr(),
             binning_capacity=int(binning_capacity), stream=torch.cuda.current_stream(dev).cuda_stream)
    if P is not None:
        f.update(P=int(P), width=int(W), height=int(H))
    return f


def _dense(t, dev):
    """The hand-off rule of every tensor these wrappers READ: float32, contiguous, 16-byte aligned and on `dev` (the device of the
    forward's buffers, where the kernel runs), made so by a copy where it is not (a camera matrix kept on the host, a column
    slice, a transposed storage, an expanded upstream gradient, a view that starts inside another tensor's storage -- the kernels
    read rotations and the per-pixel moments 16 bytes at a time).  The common case costs four tests."""
    t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _buffers_on(dev, geomBuffer, binningBuffer, imageBuffer):
    """The three buffers a forward left are read where they lie: all on `dev`, contiguous -- refused otherwise.  Their sizes and
    inner layout are the forward's own (the library reads them from the geometry header)."""
    for name, t in (("geomBuffer", geomBuffer), ("binningBuffer", binningBuffer), ("imageBuffer", imageBuffer)):
        if t.device != dev or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous tensor on {dev}, the device of the forward's state (got {t.device})")


def _int32_on(who, dev, **tensors):
    """radii, median_ids: read in place as int32 -- RuntimeError unless int32, contiguous and on `dev`."""
    for name, t in tensors.items():
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"{who}: {name} must be a contiguous int32 tensor on {dev}, got {t.dtype} on {t.device}")


def _sized(who, **tensors):
    """Every (tensor, element count) pair given by name: RuntimeError unless a present tensor has exactly that many elements --
    the kernels index these pointers by P, H and W and nothing else knows their extent."""
    for name, (t, n) in tensors.items():
        if t is not None and t.numel() != n:
            raise RuntimeError(f"{who}: {name} must have {n} elements, got {tuple(t.shape)}")


def _call(entry, args, dev, who):
    """lib().<entry>(args) with `dev` current; a refusal raises as `who`."""
    with _lib_check.on_device(dev):
        rc = getattr(_lib_check.lib(), entry)(args)
    if rc < 0:
        _lib_check.raise_for(rc, who)


def render_median(geomBuffer, binningBuffer, imageBuffer, P, image_height, image_width, *, binning_capacity=0, want_ids=True):
    """(median_depth (1, H, W) float32, median_ids (H, W) int32 or None) of the forward that left the three buffers
    (lr_render_median, on the current stream): the view-space depth and the row of the Gaussian at which each pixel's
    transmittance first falls below one half; 0 / -1 where it never does.  No autograd."""
    import torch
    H, W = int(image_height), int(image_width)
    dev = imageBuffer.device
    depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev) if want_ids else None
    a = _lib_check.MedianArgs(out_median_depth=depth.data_ptr(), out_ids=ids.data_ptr() if want_ids else None,
                              **_forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev, P, W, H))
    _call("lr_render_median", a, dev, "render_median")
    return depth, ids


def median_backward(geomBuffer, binningBuffer, imageBuffer, radii, median_ids, dL_dmedian, viewmatrix, *, binning_capacity=0,
                    accumulate_into=None):
    """dL/dmeans3D (P, 3) of the median depth (lr_median_backward): dL_dmedian (1, H, W) gathered per Gaussian through
    median_ids and taken through the view matrix's z row.  accumulate_into: a contiguous float32 (P, 3) tensor whose rows of
    visible Gaussians are added to in place (returned); else a new tensor, zero where radii <= 0."""
    import torch
    H, W = median_ids.shape
    P = radii.shape[0]
    dev = imageBuffer.device
    _int32_on("median_backward", dev, radii=radii, median_ids=median_ids)
    if median_ids.dim() != 2 or radii.dim() != 1:
        raise RuntimeError("median_backward: median_ids must be (H, W) and radii (P)")
    out = accumulate_into if accumulate_into is not None else torch.empty((P, 3), dtype=torch.float32, device=dev)
    if accumulate_into is not None and (not out.is_contiguous() or out.dtype != torch.float32 or out.numel() != 3 * P or
                                        out.device != dev):
        raise RuntimeError("median_backward: accumulate_into must be a contiguous float32 (P, 3) tensor on the forward's device")
    dL, view = _dense(dL_dmedian, dev), _dense(viewmatrix, dev)
    if dL.numel() != H * W:
        raise RuntimeError("median_backward: dL_dmedian must have H x W elements")
    _sized("median_backward", viewmatrix=(view, 16))
    a = _lib_check.MedianBackwardArgs(radii=radii.data_ptr(), ids=median_ids.data_ptr(), dL_dmedian=dL.data_ptr(),
                                      viewmatrix=view.data_ptr(), dL_dmean3D=out.data_ptr(),
                                      accumulate=1 if accumulate_into is not None else 0,
                                      **_forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev, P, W, H))
    _call("lr_median_backward", a, dev, "median_backward")
    return out


distortion_map_coefficients = _lib_check.distortion_map_coefficients
_present = lambda t: t is not None and t.numel() != 0
_ptr = lambda t: t.data_ptr() if t is not None else None


def _radii_on(who, dev, radii, P):
    """The forward's radii as the library reads them: int32 [P], contiguous, on `dev`."""
    rad = radii.contiguous()
    _sized(who, radii=(rad, P))
    _int32_on(who, dev, radii=rad)
    return rad


def _side_view(rs, P, dev, *, means3D, opacities, scales, rotations, cov3D_precomp, raw):
    """(lr_view, tensors to keep alive) of a pass behind a forward: the forward's camera (rs: its raster settings) and its geometry
    in the representation given -- scales + rotations, cov3D_precomp, or neither where the pass reads none (an empty placeholder is
    absent) -- each made _dense once and held to its element count."""
    d = lambda t, given: _dense(t, dev) if given else None
    keep = view, proj, campos, m3, op, sc, rot, cov = (
        _dense(rs.viewmatrix, dev), _dense(rs.projmatrix, dev), _dense(rs.campos, dev), _dense(means3D, dev),
        d(opacities, opacities is not None), d(scales, _present(scales)), d(rotations, _present(rotations)),
        d(cov3D_precomp, _present(cov3D_precomp)))
    _sized("the forward's view", viewmatrix=(view, 16), projmatrix=(proj, 16), campos=(campos, 3), means3D=(m3, 3 * P),
           opacities=(op, P), scales=(sc, 3 * P), rotations=(rot, 4 * P), cov3D_precomp=(cov, 6 * P))
    v = _lib_check.View(P=P, D=0, M=1, raw=1 if raw else 0, width=int(rs.image_width), height=int(rs.image_height),
                        means3D=m3.data_ptr(), opacities=_ptr(op), scales=_ptr(sc), scale_modifier=float(rs.scale_modifier),
                        rotations=_ptr(rot), cov3D_precomp=_ptr(cov), viewmatrix=view.data_ptr(), projmatrix=proj.data_ptr(),
                        campos=campos.data_ptr(), tan_fovx=float(rs.tanfovx), tan_fovy=float(rs.tanfovy))
    return v, keep


_SIDE_ACC_BITS = {"means2D": 0, "opacity": 2, "means3D": 4, "cov3D": 5, "scales": 7, "rotations": 8, "features": 9}


def _geometric_shapes(P, v):
    """{name: shape, or None for the representation not in use} of the geometric gradients of a pass whose lr_view is `v`."""
    return {"means2D": (P, 3), "opacity": (P, 1), "means3D": (P, 3), "scales": (P, 3) if v.scales else None,
            "rotations": (P, 4) if v.rotations else None, "cov3D": (P, 6) if v.cov3D_precomp else None}


def _grad_targets(who, dev, shapes, accumulate_into):
    """(out, accumulate_mask) of a side pass's backward.  shapes: {name: shape or None}; per name `out` holds None (no shape), the
    tensor accumulate_into gives for it -- contiguous float32 of that many elements on `dev`, 16-byte aligned (the kernels add
    with 16-byte accesses), RuntimeError otherwise; its bit of the mask is set -- or a new tensor, which the library writes in full."""
    out, mask = {}, 0
    for name, shape in shapes.items():
        t = (accumulate_into or {}).get(name)
        if shape is None:
            out[name] = None
        elif t is not None:
            if not t.is_contiguous() or t.dtype != torch.float32 or t.numel() != int(torch.Size(shape).numel()) or t.device != dev \
                    or t.data_ptr() % 16 != 0:
                raise RuntimeError(f"{who}: accumulate_into[{name!r}] must be a contiguous, 16-byte aligned float32 tensor of "
                                   f"{shape} on {dev}")
            out[name] = t
            mask |= 1 << _SIDE_ACC_BITS[name]
        else:
            out[name] = torch.empty(shape, dtype=torch.float32, device=dev)
    return out, mask


def _grad_fields(out, mask):
    """The gradient-output members of a side pass's backward struct, from _grad_targets' pair."""
    return dict(dL_dmean2D=_ptr(out["means2D"]), dL_dopacity=_ptr(out["opacity"]), dL_dmean3D=_ptr(out["means3D"]),
                dL_dcov3D=_ptr(out.get("cov3D")), dL_dscale=_ptr(out["scales"]), dL_drot=_ptr(out["rotations"]), accumulate_mask=mask)


def render_distortion(geomBuffer, binningBuffer, imageBuffer, P, image_height, image_width, *, distortion_map="ndc",
                      binning_capacity=0):
    """(distortion (1, H, W), moments (H, W, 4)) float32 of the forward that left the three buffers (lr_render_distortion, on the
    current stream): the depth distortion of each pixel's blended layers for the mapped depth of `distortion_map`
    (distortion_map_coefficients), and the per-pixel sums distortion_backward needs.  No autograd."""
    H, W = int(image_height), int(image_width)
    dev = imageBuffer.device
    c0, c1, c2 = distortion_map_coefficients(distortion_map)
    dist = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    mom = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    a = _lib_check.DistortionArgs(map_c0=c0, map_c1=c1, map_c2=c2, out_distortion=dist.data_ptr(), out_moments=mom.data_ptr(),
                                  **_forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev, P, W, H))
    _call("lr_render_distortion", a, dev, "render_distortion")
    return dist, mom


def distortion_backward(geomBuffer, binningBuffer, imageBuffer, dL_ddistortion, distortion, moments, rs, *, means3D,
                        opacities=None, scales=None, rotations=None, cov3D_precomp=None, raw=False, distortion_map="ndc", binning_capacity=0,
                        accumulate_into=None):
    """The distortion's gradient (lr_distortion_backward, on the current stream, behind the colour backward of the same forward).
    rs: the forward's raster settings; means3D .. cov3D_precomp: its inputs (raw=True: the stored xyz, opacity, scaling, rotation;
    the opacities are read in raw mode only, for the sigmoid's derivative).
    accumulate_into: {"means2D", "opacity", "means3D", "scales", "rotations", "cov3D": contiguous float32 tensor or None} -- a
    given tensor is ADDED to in place (rows of Gaussians that own a tile instance; the others stay untouched), a missing one is
    a new tensor written in full.  Returns the dict of the six (None for the representation not in use)."""
    who = "distortion_backward"
    dev = imageBuffer.device
    P = int(means3D.shape[0])
    H, W = int(rs.image_height), int(rs.image_width)
    c0, c1, c2 = distortion_map_coefficients(distortion_map)
    dL, dist, mom = _dense(dL_ddistortion, dev), _dense(distortion, dev), _dense(moments, dev)
    if raw and opacities is None:
        raise RuntimeError(f"{who}: raw mode needs the stored opacities")
    _sized(who, dL_ddistortion=(dL, H * W), distortion=(dist, H * W), moments=(mom, 4 * H * W))
    v, keep = _side_view(rs, P, dev, means3D=means3D, opacities=opacities, scales=scales, rotations=rotations,
                         cov3D_precomp=cov3D_precomp, raw=raw)
    out, mask = _grad_targets(who, dev, _geometric_shapes(P, v), accumulate_into)
    a = _lib_check.DistortionBackwardArgs(
        view=v, dL_ddistortion=dL.data_ptr(), moments=mom.data_ptr(), distortion=dist.data_ptr(), map_c0=c0, map_c1=c1, map_c2=c2,
        **_grad_fields(out, mask), **_forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev))
    _call("lr_distortion_backward", a, dev, who)
    del keep
    return out


def require_scale_rot(who, scales, rotations, cov3D_precomp):
    if _present(cov3D_precomp) or not _present(scales) or not _present(rotations):
        raise ValueError(f"{who}: the rendered normal map needs scales + rotations (a Gaussian given by cov3D_precomp has no normal)")


def render_normals(geomBuffer, binningBuffer, imageBuffer, radii, rs, *, means3D, scales, rotations, cov3D_precomp=None, raw=False,
                   binning_capacity=0):
    """(normals (3, H, W), gauss_normals (P, 4)) float32 of the forward that left the three buffers (lr_render_normals, on the
    current stream): N = sum_i w_i n_i over each pixel's blended layers, n_i the Gaussian's view-space normal (its shortest
    axis, turned towards the camera), and the per-Gaussian {n.xyz, sign (k + 1)} render_normals_backward needs.  rs: the
    forward's raster settings; radii: its radii.  ValueError with cov3D_precomp, before any launch.  No autograd."""
    require_scale_rot("render_normals", scales, rotations, cov3D_precomp)
    dev = imageBuffer.device
    P = int(means3D.shape[0])
    normals = torch.empty((3, int(rs.image_height), int(rs.image_width)), dtype=torch.float32, device=dev)
    gauss_normals = torch.empty((P, 4), dtype=torch.float32, device=dev)
    v, keep = _side_view(rs, P, dev, means3D=means3D, opacities=None, scales=scales, rotations=rotations, cov3D_precomp=None, raw=raw)
    rad = _radii_on("render_normals", dev, radii, P)
    a = _lib_check.NormalsRenderArgs(view=v, radii=rad.data_ptr(), out_normals=normals.data_ptr(),
                                     out_gauss_normals=gauss_normals.data_ptr(),
                                     **_forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev))
    _call("lr_render_normals", a, dev, "render_normals")
    del keep
    return normals, gauss_normals


def render_normals_backward(geomBuffer, binningBuffer, imageBuffer, dL_dnormals, normals, gauss_normals, radii, rs, *, means3D,
                            opacities=None, scales=None, rotations=None, cov3D_precomp=None, raw=False, binning_capacity=0,
                            accumulate_into=None):
    """The rendered normal map's gradient (lr_render_normals_backward, on the current stream, behind the colour backward -- and the
    distortion backward -- of the same forward).  Arguments as distortion_backward; accumulate_into: {"means2D", "opacity",
    "means3D", "scales", "rotations": tensor or None}, a given tensor is ADDED to in place, a missing one is a new tensor written in
    full.  Returns the dict of the five plus "gauss_normal": dL/dn per Gaussian (P, 3), always a new tensor."""
    who = "render_normals_backward"
    require_scale_rot(who, scales, rotations, cov3D_precomp)
    dev = imageBuffer.device
    P = int(means3D.shape[0])
    H, W = int(rs.image_height), int(rs.image_width)
    dL, nrm, gn = _dense(dL_dnormals, dev), _dense(normals, dev), _dense(gauss_normals, dev)
    if raw and opacities is None:
        raise RuntimeError(f"{who}: raw mode needs the stored opacities")
    _sized(who, dL_dnormals=(dL, 3 * H * W), normals=(nrm, 3 * H * W), gauss_normals=(gn, 4 * P))
    rad = _radii_on(who, dev, radii, P)
    v, keep = _side_view(rs, P, dev, means3D=means3D, opacities=opacities, scales=scales, rotations=rotations, cov3D_precomp=None,
                         raw=raw)
    shapes = _geometric_shapes(P, v)
    del shapes["cov3D"]
    out, mask = _grad_targets(who, dev, shapes, accumulate_into)
    out["gauss_normal"] = torch.empty((P, 3), dtype=torch.float32, device=dev)
    a = _lib_check.NormalsRenderBackwardArgs(
        view=v, dL_dnormals=dL.data_ptr(), normals=nrm.data_ptr(), gauss_normals=gn.data_ptr(), radii=rad.data_ptr(),
        dL_dgauss_normal=out["gauss_normal"].data_ptr(), **_grad_fields(out, mask),
        **_forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev))
    _call("lr_render_normals_backward", a, dev, who)
    del keep
    return out


FEATURE_MAX_CHANNELS = _lib_check.LR_FEATURE_MAX_CHANNELS


def require_features(who, features, P):
    """features as the feature-map entries take it: a float32 (P, C) tensor with 1 <= C <= FEATURE_MAX_CHANNELS -- ValueError
    otherwise, before any launch (a dtype is not converted here: a float64 or integer table handed in by mistake would be
    rendered from a silent copy whose gradient the caller never sees).  Returns C."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2:
        raise ValueError(f"{who}: features must be a (P, C) tensor")
    if features.dtype != torch.float32:
        raise ValueError(f"{who}: features must be float32, got {features.dtype}")
    if int(features.shape[0]) != int(P):
        raise ValueError(f"{who}: features has {int(features.shape[0])} rows for {int(P)} Gaussians")
    C = int(features.shape[1])
    if not 1 <= C <= FEATURE_MAX_CHANNELS:
        raise ValueError(f"{who}: features must have 1 .. {FEATURE_MAX_CHANNELS} channels, got {C}")
    return C


def render_features(geomBuffer, binningBuffer, imageBuffer, features, rs, *, binning_capacity=0):
    """feature_map (C, H, W) float32 of the forward that left the three buffers (lr_render_features, on the current stream):
    F[c] = sum_i w_i features[i, c] over each pixel's blended layers, no background term, no normalisation.  features: (P, C)
    float32, used as given; rs: the forward's raster settings.  ValueError for a wrong shape, dtype or row count -- the row count
    is checked against the P of the forward's geometry buffer by the caller (the operator passes its means3D's) -- before any
    launch.  No autograd."""
    dev = imageBuffer.device
    P = int(features.shape[0]) if isinstance(features, torch.Tensor) and features.dim() == 2 else -1
    C = require_features("render_features", features, P)
    H, W = int(rs.image_height), int(rs.image_width)
    f = _dense(features, dev)
    out = torch.empty((C, H, W), dtype=torch.float32, device=dev)
    a = _lib_check.FeatureRenderArgs(view=_lib_check.View(P=P, D=0, M=1, width=W, height=H), features=f.data_ptr(), channels=C,
                                     out_features=out.data_ptr(),
                                     **_forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev))
    _call("lr_render_features", a, dev, "render_features")
    del f
    return out


def render_features_backward(geomBuffer, binningBuffer, imageBuffer, dL_dout_features, out_features, features, radii, rs, *,
                             means3D, slots, opacities=None, scales=None, rotations=None, cov3D_precomp=None, raw=False,
                             binning_capacity=0, accumulate_into=None):
    """The feature map's gradient (lr_render_features_backward, on the current stream, behind the colour backward -- and the other
    passes' backwards -- of the same forward).  Arguments as distortion_backward; slots: the bound of the forward's instance
    count the workspace is sized by (the forward's num_rendered in exact mode; async mode takes binning_capacity);
    accumulate_into: {"means2D", "opacity", "means3D", "scales", "rotations", "cov3D", "features": tensor or None}, a given tensor
    is ADDED to in place, a missing one is a new tensor written in full.  Returns the dict of the seven (None for the
    representation not in use)."""
    who = "render_features_backward"
    dev = imageBuffer.device
    P = int(means3D.shape[0])
    C = require_features(who, features, P)
    H, W = int(rs.image_height), int(rs.image_width)
    dL, val, f = _dense(dL_dout_features, dev), _dense(out_features, dev), _dense(features, dev)
    if raw and opacities is None:
        raise RuntimeError(f"{who}: raw mode needs the stored opacities")
    _sized(who, dL_dout_features=(dL, C * H * W), out_features=(val, C * H * W))
    rad = _radii_on(who, dev, radii, P)
    v, keep = _side_view(rs, P, dev, means3D=means3D, opacities=opacities, scales=scales, rotations=rotations,
                         cov3D_precomp=cov3D_precomp, raw=raw)
    out, mask = _grad_targets(who, dev, dict(_geometric_shapes(P, v), features=(P, C)), accumulate_into)
    bound = int(binning_capacity) if int(binning_capacity) > 0 else max(int(slots), 1)
    ws_bytes = int(_lib_check.lib().lr_features_workspace_bytes(bound, C))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    a = _lib_check.FeatureRenderBackwardArgs(
        view=v, features=f.data_ptr(), channels=C, dL_dout_features=dL.data_ptr(), out_features=val.data_ptr(), radii=rad.data_ptr(),
        dL_dfeatures=out["features"].data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws_bytes, **_grad_fields(out, mask),
        **_forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev))
    _call("lr_render_features_backward", a, dev, who)
    del keep, ws
    return out


def render_geometry(geomBuffer, binningBuffer, imageBuffer, radii, rs, *, means3D, scales, rotations, cov3D_precomp=None, raw=False,
                    distortion_map="ndc", binning_capacity=0):
    """(distortion (1, H, W), moments (H, W, 4), normals (3, H, W), gauss_normals (P, 4)): render_distortion and render_normals in
    ONE tile walk (lr_render_geometry, on the current stream) -- the pass the multi-view step runs.  Arguments as render_normals,
    with render_distortion's distortion_map.  ValueError with cov3D_precomp, before any launch.  No autograd."""
    require_scale_rot("render_geometry", scales, rotations, cov3D_precomp)
    dev = imageBuffer.device
    P = int(means3D.shape[0])
    H, W = int(rs.image_height), int(rs.image_width)
    c0, c1, c2 = distortion_map_coefficients(distortion_map)
    dist = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    mom = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    normals = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    gauss_normals = torch.empty((P, 4), dtype=torch.float32, device=dev)
    v, keep = _side_view(rs, P, dev, means3D=means3D, opacities=None, scales=scales, rotations=rotations, cov3D_precomp=None, raw=raw)
    rad = _radii_on("render_geometry", dev, radii, P)
    a = _lib_check.GeometryArgs(view=v, radii=rad.data_ptr(), map_c0=c0, map_c1=c1, map_c2=c2, out_distortion=dist.data_ptr(),
                                out_moments=mom.data_ptr(), out_normals=normals.data_ptr(), out_gauss_normals=gauss_normals.data_ptr(),
                                **_forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev))
    _call("lr_render_geometry", a, dev, "render_geometry")
    del keep
    return dist, mom, normals, gauss_normals


def geometry_backward(geomBuffer, binningBuffer, imageBuffer, dL_ddistortion, distortion, moments, dL_dnormals, normals,
                      gauss_normals, radii, rs, *, means3D, opacities=None, scales=None, rotations=None, cov3D_precomp=None, raw=False,
                      distortion_map="ndc", binning_capacity=0, accumulate_into=None):
    """The gradient of both maps of render_geometry in one per-tile kernel and one per-Gaussian pass (lr_geometry_backward, on the
    current stream, behind the colour backward of the same forward).  dL_ddistortion: (1, H, W), a Python number (the upstream of
    every pixel) or None; dL_dnormals: (3, H, W) or None; an absent upstream contributes nothing.  The other arguments and the
    returned dict are render_normals_backward's."""
    who = "geometry_backward"
    require_scale_rot(who, scales, rotations, cov3D_precomp)
    dev = imageBuffer.device
    P = int(means3D.shape[0])
    H, W = int(rs.image_height), int(rs.image_width)
    c0, c1, c2 = distortion_map_coefficients(distortion_map)
    scalar = float(dL_ddistortion) if isinstance(dL_ddistortion, (int, float)) else 0.0
    dD = _dense(dL_ddistortion, dev) if isinstance(dL_ddistortion, torch.Tensor) else None
    dN = _dense(dL_dnormals, dev) if dL_dnormals is not None else None
    dist, mom, nrm, gn = _dense(distortion, dev), _dense(moments, dev), _dense(normals, dev), _dense(gauss_normals, dev)
    if raw and opacities is None:
        raise RuntimeError(f"{who}: raw mode needs the stored opacities")
    _sized(who, dL_ddistortion=(dD, H * W), distortion=(dist, H * W), moments=(mom, 4 * H * W), dL_dnormals=(dN, 3 * H * W),
           normals=(nrm, 3 * H * W), gauss_normals=(gn, 4 * P))
    rad = _radii_on(who, dev, radii, P)
    v, keep = _side_view(rs, P, dev, means3D=means3D, opacities=opacities, scales=scales, rotations=rotations, cov3D_precomp=None,
                         raw=raw)
    shapes = _geometric_shapes(P, v)
    del shapes["cov3D"]
    out, mask = _grad_targets(who, dev, shapes, accumulate_into)
    out["gauss_normal"] = torch.empty((P, 3), dtype=torch.float32, device=dev)
    a = _lib_check.GeometryBackwardArgs(
        view=v, dL_ddistortion=_ptr(dD), dL_ddistortion_scalar=scalar, moments=mom.data_ptr(), distortion=dist.data_ptr(),
        map_c0=c0, map_c1=c1, map_c2=c2, dL_dnormals=_ptr(dN), normals=nrm.data_ptr(), gauss_normals=gn.data_ptr(),
        radii=rad.data_ptr(), dL_dgauss_normal=out["gauss_normal"].data_ptr(), **_grad_fields(out, mask),
        **_forward_state(geomBuffer, binningBuffer, imageBuffer, binning_capacity, dev))
    _call("lr_geometry_backward", a, dev, who)
    del keep
    return out


# forward + backward of one view in one call for a caller that holds dL/dcolor up front; [] = an input does not qualify
rasterize_view_step = _C_ext.rasterize_view_step
last_num_rendered = _C_ext.last_num_rendered


def request_early_header():
    """The next async-mode forward on this thread posts a header ticket right after its compaction scan (lr_request_early_header)."""
    _C_ext.request_early_header()


def take_early_ticket():
    """Ticket of that early header copy, or -1."""
    return _C_ext.take_early_ticket()


def last_forward_ticket():
    """Ticket (for header_poll) of the last async-mode forward on this thread, from the library's forward log: costs nothing --
    the scan kernel itself leaves the header in host-visible memory (lr_forward_ticket); -1 if there was none."""
    return _C_ext.last_forward_ticket()


def header_post(geomBuffer):
    """Non-blocking read-back of a forward's header on the current stream (lr_header_post); returns a ticket."""
    return _C_ext.header_post(geomBuffer)


def header_poll(ticket, block=False):
    """None while the read-back is in flight (block=False), else the 8 header words (the ticket is released)."""
    return _C_ext.header_poll(ticket, block)
