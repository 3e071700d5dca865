"""The 3D smoothing filter of Mip-Splatting (Yu et al., "Mip-Splatting: Alias-free 3D Gaussian Splatting", 2024) for a
GaussianModel on the MI355X: the half of Mip-Splatting that `config.set_antialiasing` (the 2D Mip filter) is not.  The two are
independent; the paper uses both.

    f = filter3d.compute_filter_3d(model.get_xyz, train_cams)      # [P,1]; again after every change of the set of Gaussians
    view = filter3d.filtered(model, f)
    render_raw(cam, view)            # or render(cam, view), ViewBatch.run(..., view.get_opacity, view.get_scaling, ...),
    densify.save_ply(view, path)     # a "fused" .ply any viewer renders correctly without knowing about the filter

Every Gaussian is convolved with an isotropic Gaussian low-pass of standard deviation filter_k = sqrt(variance) * d_k, where
d_k = min over the cameras that see Gaussian k of (view-space z) / fx is the reciprocal of the highest sampling rate any training
camera has of it: s' = sqrt(s^2 + f^2) per axis and the opacity times sqrt(prod s^2 / prod s'^2), so that a camera closer than
every training view does not find needles thinner than anything the training views could have resolved.  The definitions, the
visibility test and the float32 operation order are in include/lucid_raster.h (lr_filter3d_*) and DESIGN.md section 4b-F3D.
d_k is the paper's: the minimum of z / fx over the cameras.  Mip-Splatting's released code takes the minimum z and the maximum
focal length separately, which is the same when all cameras share a focal length and a smaller filter otherwise.

The filter acts on the stored parameters before a rasterizer sees them, and its result can be expressed in the stored domain
(log scale, logit opacity) as well as in the activated one, so every existing path consumes it unchanged and no rasterizer kernel
knows about it.  The arithmetic is in csrc/filter3d.hip, forward and backward, one launch each; there is no CPU path.

Not covered: the filter inside the raw preprocess kernels, `install()` (the drop-in patches do not apply it), and carrying filter
rows through `densify.RowStore` -- recompute the filter after a densification instead (a filter whose length is not the model's
raises ValueError before anything is launched).
"""
import math

import torch

from . import _lib


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _f32(t, what, numel=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"luciddreamer_amd.filter3d: {what} must be on a HIP device (no CPU path)")
    if t.dtype != torch.float32 or (numel is not None and t.numel() != numel):
        raise RuntimeError(f"luciddreamer_amd.filter3d: {what} must be a float32 tensor" +
                           (f" of {numel} elements" if numel is not None else ""))
    return t.detach().contiguous()


def pack_cameras(cams, device):
    """[V,20] float32 on `device`: per camera the 16 floats of world_view_transform (row-vector convention, as stored), then
    fx = W / (2 tan(FoVx / 2)), fy = H / (2 tan(FoVy / 2)), W, H.  `cams`: objects with the MiniCam / reference Camera field names
    (world_view_transform, FoVx, FoVy, image_width, image_height)."""
    cams = list(cams)
    out = torch.empty((len(cams), 20), dtype=torch.float32)
    for n, c in enumerate(cams):
        W, H = int(c.image_width), int(c.image_height)
        out[n, :16] = c.world_view_transform.detach().to("cpu", torch.float32).reshape(16)
        out[n, 16] = W / (2.0 * math.tan(float(c.FoVx) * 0.5))
        out[n, 17] = H / (2.0 * math.tan(float(c.FoVy) * 0.5))
        out[n, 18], out[n, 19] = W, H
    return out.to(device)


def compute_filter_3d(xyz, cams_or_packed, variance=0.2, return_seen=False):
    """filter_3D [P,1] float32 of the Gaussians at `xyz` [P,3] for the training cameras (a list of cameras or pack_cameras'
    tensor), on the current stream, without a host synchronisation.  A Gaussian no camera sees gets the largest filter in use;
    if none is seen at all (no cameras included) every filter is 0.  return_seen: (filter_3D, seen [P] bool)."""
    P = int(xyz.shape[0])
    xyz = _f32(xyz, "xyz", 3 * P)
    dev = xyz.device
    packed = cams_or_packed if isinstance(cams_or_packed, torch.Tensor) else pack_cameras(cams_or_packed, dev)
    if packed.dim() != 2 or packed.shape[1] != 20:
        raise ValueError("luciddreamer_amd.filter3d: packed cameras must be [V,20] (pack_cameras)")
    packed = _f32(packed, "the packed cameras")
    if packed.device != dev:
        raise RuntimeError("luciddreamer_amd.filter3d: xyz and the packed cameras must be on the same device")
    variance = float(variance)
    if not (math.isfinite(variance) and variance >= 0.0):
        raise ValueError("luciddreamer_amd.filter3d: variance must be finite and >= 0")
    V = int(packed.shape[0])
    L = _lib.lib()
    out = torch.empty((P, 1), dtype=torch.float32, device=dev)
    seen = torch.empty((P,), dtype=torch.uint8, device=dev) if return_seen else None
    ws = torch.empty((L.lr_filter3d_workspace_bytes(P),), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        rc = L.lr_filter3d_update(P, V, xyz.data_ptr() if P else None, packed.data_ptr() if V else None, variance,
                                  out.data_ptr() if P else None, seen.data_ptr() if return_seen and P else None, ws.data_ptr(),
                                  _stream(dev))
    if rc < 0:
        _lib.raise_for(rc, "lr_filter3d_update")
    return (out, seen.bool()) if return_seen else out


def _check_apply(raw_scaling, raw_opacity, filter_3D):
    P = int(raw_scaling.shape[0])
    if not isinstance(filter_3D, torch.Tensor) or filter_3D.numel() != P:
        n = filter_3D.numel() if isinstance(filter_3D, torch.Tensor) else "no"
        raise ValueError(f"luciddreamer_amd.filter3d: the filter has {n} rows, the model {P}: recompute it "
                         "(compute_filter_3d) after every change of the set of Gaussians")
    _f32(raw_scaling, "scaling", 3 * P), _f32(raw_opacity, "opacity", P), _f32(filter_3D, "filter_3D", P)
    if not (raw_scaling.device == raw_opacity.device == filter_3D.device):
        raise RuntimeError("luciddreamer_amd.filter3d: scaling, opacity and filter_3D must be on the same device")
    return P


class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw_scaling, raw_opacity, filter_3D, activated):
        P = int(raw_scaling.shape[0])
        s, o, f = _f32(raw_scaling, "scaling"), _f32(raw_opacity, "opacity"), _f32(filter_3D, "filter_3D")
        dev = s.device
        out_s, out_o = torch.empty_like(s), torch.empty_like(o)
        if P:
            with _lib.on_device(dev):
                rc = _lib.lib().lr_filter3d_apply_forward(P, s.data_ptr(), o.data_ptr(), f.data_ptr(), int(activated),
                                                          out_s.data_ptr(), out_o.data_ptr(), _stream(dev))
            if rc < 0:
                _lib.raise_for(rc, "lr_filter3d_apply_forward")
        ctx.activated = int(activated)
        ctx.save_for_backward(s, o, f)
        ctx.set_materialize_grads(False)                # an output nobody used arrives as None = the kernel's NULL upstream
        return out_s, out_o

    @staticmethod
    def backward(ctx, g_s, g_o):
        s, o, f = ctx.saved_tensors
        d_s, d_o = backward(s, o, f, g_s, g_o, activated=ctx.activated)
        return d_s, d_o, None, None


def backward(raw_scaling, raw_opacity, filter_3D, grad_scaling=None, grad_opacity=None, activated=False):
    """lr_filter3d_apply_backward on tensors: (dL/draw_scaling, dL/draw_opacity) from the upstream gradients of apply()'s two
    outputs (None = zero).  What apply()'s autograd node runs."""
    P = _check_apply(raw_scaling, raw_opacity, filter_3D)
    s, o, f = _f32(raw_scaling, "scaling"), _f32(raw_opacity, "opacity"), _f32(filter_3D, "filter_3D")
    g_s = _f32(grad_scaling, "the scaling gradient", 3 * P) if grad_scaling is not None else None
    g_o = _f32(grad_opacity, "the opacity gradient", P) if grad_opacity is not None else None
    dev = s.device
    if any(g is not None and g.device != dev for g in (g_s, g_o)):
        raise RuntimeError("luciddreamer_amd.filter3d: the upstream gradients must be on the device of the parameters")
    d_s, d_o = torch.empty_like(s), torch.empty_like(o)
    if P:
        with _lib.on_device(dev):
            rc = _lib.lib().lr_filter3d_apply_backward(P, s.data_ptr(), o.data_ptr(), f.data_ptr(), int(bool(activated)),
                                                       g_s.data_ptr() if g_s is not None else None,
                                                       g_o.data_ptr() if g_o is not None else None,
                                                       d_s.data_ptr(), d_o.data_ptr(), _stream(dev))
        if rc < 0:
            _lib.raise_for(rc, "lr_filter3d_apply_backward")
    return d_s, d_o


def apply(raw_scaling, raw_opacity, filter_3D, activated=False):
    """The filter applied to stored parameters: raw_scaling [P,3] (log), raw_opacity [P,1] (logit), filter_3D [P,1] or [P].
    activated=False: (log s', logit o'), the stored domain -- what render_raw, save_ply and every raw-parameter path take; rows
    with a filter of 0 keep their bits.  activated=True: (s', o') -- what render, ViewBatch.run and the getters take.
    Differentiable in raw_scaling and raw_opacity (one HIP kernel each way); the filter is a constant."""
    _check_apply(raw_scaling, raw_opacity, filter_3D)
    return _Apply.apply(raw_scaling, raw_opacity, filter_3D, bool(activated))


class FilteredView:
    """What filtered() returns: `model` with the 3D filter applied to what it shows of its scale and opacity."""

    def __init__(self, model, filter_3D):
        _check_apply(model._scaling, model._opacity, filter_3D)
        object.__setattr__(self, "_model", model)
        object.__setattr__(self, "filter_3D", filter_3D)
        object.__setattr__(self, "_pairs", {})

    def _pair(self, activated):
        if activated not in self._pairs:
            m = self._model
            self._pairs[activated] = apply(m._scaling, m._opacity, self.filter_3D, activated=activated)
        return self._pairs[activated]

    @property
    def _scaling(self):
        return self._pair(False)[0]

    @property
    def _opacity(self):
        return self._pair(False)[1]

    @property
    def get_scaling(self):
        return self._pair(True)[0]

    @property
    def get_opacity(self):
        return self._pair(True)[1]

    def get_covariance(self, scaling_modifier=1):
        raise NotImplementedError("luciddreamer_amd.filter3d: a filtered view has no get_covariance (compute_cov3D_python); "
                                  "pass its scales and rotations to the rasterizer")

    def __getattr__(self, name):                        # everything else is the model's
        return getattr(object.__getattribute__(self, "_model"), name)

    def __setattr__(self, name, value):
        raise AttributeError("luciddreamer_amd.filter3d: a filtered view is read-only; change the model and take a new view")


def filtered(model, filter_3D):
    """A read-only duck-typed view of `model` (GaussianCloud, TrainableCloud, a reference GaussianModel) under the filter:
    `_scaling` / `_opacity` are the stored-domain outputs of apply(), `get_scaling` / `get_opacity` the activated ones, each pair
    computed at most once per view object; every other attribute is the model's.  Gradients reach the model's own parameters
    through autograd.  Take a new view after every optimizer step (the view caches what it computed from the parameters)."""
    return FilteredView(model, filter_3D)
