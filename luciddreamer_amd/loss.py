"""Fused photometric loss of the training loop on the MI355X.

    loss = l1_dssim_loss(image, gt, lambda_dssim)      # == (1-l)*l1_loss(image, gt) + l*(1 - ssim(image, gt))

is what /root/reference/luciddreamer.py:301-304 computes with utils/loss.py's l1_loss (:18-19) and ssim (:37-69).
`l1_loss` and `ssim` with the reference's names and meaning are provided as well.  One HIP kernel pass forward and one
backward (luciddreamer_amd/csrc/loss.hip) through the C-ABI (lr_l1_dssim_forward / lr_l1_dssim_backward); no CPU or
PyTorch fallback.  Gradients flow to `image` only (the target is data).
"""
import torch

from . import _lib

_WS_BYTES = {}                      # (size query's name, dims) -> its answer: a C call per forward otherwise


def _ws_bytes(query, *dims):
    n = _WS_BYTES.get((query, dims))
    if n is None:
        n = _WS_BYTES[(query, dims)] = int(getattr(_lib.lib(), query)(*dims))
    return n


def _call(fn, what, dev, *args):
    """fn(*args, the current stream of dev) with dev the current HIP device; a refusal raises as `what`."""
    with _lib.on_device(dev):
        rc = fn(*args, torch.cuda.current_stream(dev).cuda_stream)
    if rc < 0:
        _lib.raise_for(rc, what)


def _weight(t, dev):
    """An upstream gradient as the one-float device tensor the kernels read: as it is when autograd already hands over a float32
    scalar on the device (the usual case: three tensor ops saved per backward), converted otherwise."""
    if t is None:
        return torch.zeros(1, device=dev)
    if t.dtype is torch.float32 and t.device == dev and t.numel() == 1 and t.is_contiguous():
        return t
    return t.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()


def _image_pair(image, gt):
    """(image, gt, C, H, W) of a float32 device pair of one [..., H, W] shape, contiguous."""
    if not image.is_cuda or not gt.is_cuda:
        raise RuntimeError("luciddreamer_amd.loss: image and gt must be on a HIP device (no CPU path)")
    if image.shape != gt.shape or image.dim() < 2:
        raise RuntimeError(f"image {tuple(image.shape)} and gt {tuple(gt.shape)} must have the same [..., H, W] shape")
    if image.device != gt.device:
        raise RuntimeError(f"image ({image.device}) and gt ({gt.device}) must be on one device")
    if image.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError("image and gt must be float32")
    x, g = image.contiguous(), gt.contiguous()
    H, W = int(x.shape[-2]), int(x.shape[-1])
    return x, g, x.numel() // (H * W), H, W


def _plane(t, name, what):
    """A float32 device plane [1,H,W] or [H,W], contiguous."""
    if not t.is_cuda:
        raise RuntimeError(f"luciddreamer_amd.loss.{what}: {name} must be on a HIP device (no CPU path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32")
    if not (t.dim() == 2 or (t.dim() == 3 and t.shape[0] == 1)):
        raise RuntimeError(f"{name} {tuple(t.shape)} must be [1,H,W] or [H,W]")
    return t.contiguous()


def _depth_pair(depth, target, what):
    """(depth, target, H, W) of two planes of one H, W."""
    d, t = _plane(depth, "depth", what), _plane(target, "target", what)
    if d.shape[-2:] != t.shape[-2:] or d.device != t.device:
        raise RuntimeError(f"depth {tuple(depth.shape)} and target {tuple(target.shape)} must be [1,H,W] or [H,W] of one H, W, "
                           "on one device")
    return d, t, int(d.shape[-2]), int(d.shape[-1])


def _mask_hw(mask, H, W, dev):
    if not mask.is_cuda or mask.device != dev or mask.dtype != torch.float32:
        raise RuntimeError("mask must be a float32 tensor on the device of the image")
    if tuple(mask.shape) not in ((H, W), (1, H, W)):
        raise RuntimeError(f"mask {tuple(mask.shape)} must be [1,H,W] or [H,W] with H,W = {H},{W}")
    return mask.contiguous()


def _pair_forward(ctx, what, image, gt, lam, mask=None):
    """One lr_l1_dssim_forward (lr_masked_l1_dssim_forward with a mask): {loss, l1, ssim} on the device, and on ctx what the
    three colour backwards read."""
    x, g, C, H, W = _image_pair(image, gt)
    dev = x.device
    m = None if mask is None else _mask_hw(mask, H, W, dev)
    L = _lib.lib()
    out3 = torch.empty((3,), dtype=torch.float32, device=dev)
    ws = torch.empty((_ws_bytes("lr_loss_workspace_bytes", C, H, W),), dtype=torch.uint8, device=dev)
    if m is None:
        _call(L.lr_l1_dssim_forward, what, dev, C, H, W, x.data_ptr(), g.data_ptr(), lam, out3.data_ptr(), ws.data_ptr(), ws.numel())
        ctx.save_for_backward(x, g, ws)
    else:
        _call(L.lr_masked_l1_dssim_forward, what, dev, C, H, W, x.data_ptr(), g.data_ptr(), m.data_ptr(), lam, out3.data_ptr(),
              ws.data_ptr(), ws.numel())
        ctx.save_for_backward(x, g, m, ws)
    ctx.lam, ctx.dims, ctx.in_shape = lam, (C, H, W), image.shape
    return out3


class _L1DSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, lambda_dssim):
        out3 = _pair_forward(ctx, "l1_dssim_loss", image, gt, float(lambda_dssim))
        ctx.parts = out3                      # {loss, l1, ssim}, device
        return out3[0]

    @staticmethod
    def backward(ctx, grad_out):
        x, g, ws = ctx.saved_tensors
        dev = x.device
        up = _weight(grad_out, dev)
        grad = torch.empty_like(x)
        _call(_lib.lib().lr_l1_dssim_backward, "l1_dssim_loss backward", dev, *ctx.dims, x.data_ptr(), g.data_ptr(), ctx.lam,
              up.data_ptr(), ws.data_ptr(), grad.data_ptr())
        return grad.view(ctx.in_shape), None, None


def l1_dssim_loss(image, gt, lambda_dssim=0.2):
    """(1 - lambda) * mean|image - gt| + lambda * (1 - SSIM(image, gt)); image, gt: [C,H,W] (or [B,C,H,W])."""
    return _L1DSSIM.apply(image, gt, lambda_dssim)


def l1_loss(network_output, gt):
    """utils/loss.py:18-19."""
    return _L1DSSIM.apply(network_output, gt, 0.0)


def ssim(img1, img2, window_size=11, size_average=True):
    """utils/loss.py:37-46 (window 11, averaged over everything -- the only configuration the training loop uses)."""
    if window_size != 11 or not size_average:
        raise NotImplementedError("fused ssim supports window_size=11, size_average=True")
    return 1.0 - _L1DSSIM.apply(img1, img2, 1.0)


class _L1SSIMPair(torch.autograd.Function):
    """(l1, ssim) of one image pair from ONE forward pass, for callers that weight the two means themselves
    (/root/reference/luciddreamer.py:301-303: `(1 - l) * l1_loss(image, gt) + l * (1 - ssim(image, gt))`); the backward takes
    both grad_outputs as device scalars (lr_l1_dssim_backward_weights)."""

    @staticmethod
    def forward(ctx, image, gt):
        out3 = _pair_forward(ctx, "l1 / ssim pair", image, gt, 0.0)
        return out3[1], out3[2]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        x, g, ws = ctx.saved_tensors
        dev = x.device
        w1, w2 = _weight(g_l1, dev), _weight(g_ssim, dev)
        grad = torch.empty_like(x)
        _call(_lib.lib().lr_l1_dssim_backward_weights, "l1 / ssim pair backward", dev, *ctx.dims, x.data_ptr(), g.data_ptr(),
              w1.data_ptr(), w2.data_ptr(), ws.data_ptr(), grad.data_ptr())
        return grad.view(ctx.in_shape), None


class PairedLoss:
    """`l1_loss` and `ssim` with the reference's signatures that share ONE kernel pass when they are called, in either order,
    on the same (image, gt) tensors -- which is what the training loop does.  luciddreamer_amd.install() puts a pair of these
    in place of utils/loss.py's functions.  A call with other tensors (or ssim with another window) computes on its own."""

    def __init__(self, fallback_l1=None, fallback_ssim=None):
        """fallback_*: what a call the shared pass does not cover is handed to (install() passes the functions it replaces, so
        the caller's own code keeps serving other window sizes, per-image means, host tensors); without one, l1 of anything
        else is the reference's expression and such an ssim call raises."""
        self._key, self._pair = None, None
        self._fallback_l1, self._fallback_ssim = fallback_l1, fallback_ssim

    @staticmethod
    def _fusable(a, b):
        return (torch.is_tensor(a) and torch.is_tensor(b) and a.is_cuda and b.is_cuda and a.shape == b.shape and a.dim() >= 3
                and a.shape[-3] == 3 and a.dtype == torch.float32 and b.dtype == torch.float32)

    def _get(self, a, b):
        # the pending pair is keyed on the tensor OBJECTS (held here until the second call or the next key: an id() alone can
        # be re-used by a later tensor at the same allocator address once the first is gone -- eval loops under no_grad) and
        # their versions
        k = self._key
        if (k is not None and self._pair is not None and k[0] is a and k[1] is b and k[2] == a._version
                and k[3] == b._version and k[4] == a.data_ptr() and k[5] == b.data_ptr()):
            pair, self._key, self._pair = self._pair, None, None       # second of the two calls: hand out and forget
            return pair
        self._key, self._pair = None, None                             # another pair: drop the graph / workspace of the old one
        pair = _L1SSIMPair.apply(a, b)
        self._key, self._pair = (a, b, a._version, b._version, a.data_ptr(), b.data_ptr()), pair
        return pair

    def l1_loss(self, network_output, gt):
        # only what the loop pairs with ssim goes through the shared pass: an RGB image against its target.  Anything else
        # (a depth map, a vector) is the reference's own expression, utils/loss.py:18-19
        if not self._fusable(network_output, gt) or network_output.dim() != 3:
            if self._fallback_l1 is not None:
                return self._fallback_l1(network_output, gt)
            return torch.abs(network_output - gt).mean()
        return self._get(network_output, gt)[0]

    def ssim(self, img1, img2, window_size=11, size_average=True):
        if window_size != 11 or not size_average or not self._fusable(img1, img2):
            if self._fallback_ssim is not None:
                return self._fallback_ssim(img1, img2, window_size, size_average)
            raise NotImplementedError("fused ssim: float32 [..., 3, H, W] device tensors, window_size=11, size_average=True")
        return self._get(img1, img2)[1]


def _plane_forward(fn, query, what, n_out, H, W, a, b, weight):
    """One forward of a plane term over the planes a, b: (out [n_out], workspace)."""
    dev = a.device
    out = torch.empty((n_out,), dtype=torch.float32, device=dev)
    ws = torch.empty((_ws_bytes(query, H, W),), dtype=torch.uint8, device=dev)
    _call(fn, what, dev, H, W, a.data_ptr(), b.data_ptr(), weight, out.data_ptr(), ws.data_ptr(), ws.numel())
    return out, ws


class _DepthL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, target, weight):
        d, t, H, W = _depth_pair(depth, target, "depth_l1")
        out, _ = _plane_forward(_lib.lib().lr_depth_l1_forward, "lr_depth_l1_workspace_bytes", "depth_l1", 1, H, W, d, t,
                                float(weight))
        ctx.save_for_backward(d, t)
        ctx.weight, ctx.dims, ctx.in_shape = float(weight), (H, W), depth.shape
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        d, t = ctx.saved_tensors
        dev = d.device
        up = _weight(grad_out, dev)
        grad = torch.empty_like(d)
        _call(_lib.lib().lr_depth_l1_backward, "depth_l1 backward", dev, *ctx.dims, d.data_ptr(), t.data_ptr(), ctx.weight,
              up.data_ptr(), grad.data_ptr())
        return grad.view(ctx.in_shape), None, None


def depth_l1(depth, target, weight=1.0):
    """weight * mean over all H*W pixels of |depth - target| where target > 0 (a target that is not > 0, NaN included,
    contributes nothing); depth, target: [1,H,W] or [H,W] float32.  One HIP pass forward (per-workgroup partial sums, reduced in
    a fixed order in double: bit-repeatable) and one elementwise pass backward (lr_depth_l1_forward / lr_depth_l1_backward).
    Gradients flow to `depth` only (the target is data)."""
    return _DepthL1.apply(depth, target, weight)


def _pearson_forward(depth, target, weight, what):
    """(d, t, out {loss, rho}, workspace) of one lr_depth_pearson_forward."""
    d, t, H, W = _depth_pair(depth, target, what)
    out, ws = _plane_forward(_lib.lib().lr_depth_pearson_forward, "lr_depth_pearson_workspace_bytes", what, 2, H, W, d, t,
                             float(weight))
    return d, t, out, ws


class _DepthPearson(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, target, weight):
        d, t, out, ws = _pearson_forward(depth, target, weight, "depth_pearson")
        ctx.save_for_backward(d, t, ws)       # the backward reads the coefficient record the forward left in the workspace
        ctx.weight, ctx.in_shape = float(weight), depth.shape
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        d, t, ws = ctx.saved_tensors
        dev = d.device
        up = _weight(grad_out, dev)
        grad = torch.empty_like(d)
        _call(_lib.lib().lr_depth_pearson_backward, "depth_pearson backward", dev, int(d.shape[-2]), int(d.shape[-1]), d.data_ptr(),
              t.data_ptr(), ctx.weight, up.data_ptr(), ws.data_ptr(), ws.numel(), grad.data_ptr())
        return grad.view(ctx.in_shape), None, None


def depth_pearson(depth, target, weight=1.0):
    """weight * (1 - rho), rho the Pearson correlation of depth and target over the pixels whose target is > 0 (a target that is
    not > 0, NaN included, is left out, as in depth_l1); depth, target: [1,H,W] or [H,W] float32.  Invariant to target ->
    a * target + b with a > 0: the term for ESTIMATED (monocular) depth, which is right up to a per-frame scale and shift.
    Without a correlation (fewer than two valid pixels, constant depth or constant target on them) the loss and the gradient are
    exactly 0.  Three small HIP kernels (lr_depth_pearson_forward / _backward): the sums in double from the pixel on, reduced in
    a fixed order -- bit-repeatable.  Gradients flow to `depth` only (the target is data)."""
    return _DepthPearson.apply(depth, target, weight)


def depth_correlation(depth, target):
    """rho of depth_pearson (0 when there is none), a 0-dim device tensor without a gradient: for logging."""
    with torch.no_grad():
        return _pearson_forward(depth.detach(), target, 1.0, "depth_correlation")[2][1]


# ---- mask supervision: a colour loss only where the frame has content, a penalty on alpha in its holes ----
def content_mask(gt):
    """float32 [1,H,W] mask of the pixels of a target frame [C,H,W] where any channel is non-zero: LucidDreamer's `maskj`
    rebuilt from the frame (generate_pcd sets every pixel the projected cloud left empty to exact zero).  A genuinely black
    content pixel counts as a hole.  A one-time step during setup: a torch expression."""
    if gt.dim() != 3:
        raise RuntimeError(f"content_mask: gt must be [C,H,W], got {tuple(gt.shape)}")
    return (gt != 0).any(dim=0, keepdim=True).to(torch.float32)


class _MaskedL1DSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, mask, lambda_dssim):
        return _pair_forward(ctx, "masked_l1_dssim", image, gt, float(lambda_dssim), mask)[0]

    @staticmethod
    def backward(ctx, grad_out):
        x, g, m, ws = ctx.saved_tensors
        dev = x.device
        up = _weight(grad_out, dev)
        grad = torch.empty_like(x)
        _call(_lib.lib().lr_masked_l1_dssim_backward, "masked_l1_dssim backward", dev, *ctx.dims, x.data_ptr(), g.data_ptr(),
              m.data_ptr(), ctx.lam, up.data_ptr(), ws.data_ptr(), grad.data_ptr())
        return grad.view(ctx.in_shape), None, None, None


def masked_l1_dssim(image, gt, mask, lambda_dssim=0.2):
    """l1_dssim_loss(mask * image, mask * gt, lambda_dssim): the fused L1 + DSSIM of the masked pair (mean over all C*H*W);
    image, gt [C,H,W], mask [1,H,W] or [H,W] in [0, 1] (content_mask), shared by the channels.  The gradient flows to `image`:
    mask * dL/d(mask * image).  An all-ones mask gives l1_dssim_loss's bits.  HIP in both directions, no host synchronisation
    (lr_masked_l1_dssim_forward / _backward)."""
    return _MaskedL1DSSIM.apply(image, gt, mask, lambda_dssim)


class _AlphaHole(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, mask, weight):
        a = _plane(alpha, "alpha", "alpha_hole")
        H, W = int(a.shape[-2]), int(a.shape[-1])
        m = _mask_hw(mask, H, W, a.device)
        out, _ = _plane_forward(_lib.lib().lr_alpha_hole_forward, "lr_alpha_hole_workspace_bytes", "alpha_hole", 1, H, W, a, m,
                                float(weight))
        ctx.save_for_backward(m)
        ctx.weight, ctx.dims, ctx.in_shape = float(weight), (H, W), alpha.shape
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        m, = ctx.saved_tensors
        dev = m.device
        up = _weight(grad_out, dev)
        grad = torch.empty(ctx.in_shape, dtype=torch.float32, device=dev)
        _call(_lib.lib().lr_alpha_hole_backward, "alpha_hole backward", dev, *ctx.dims, m.data_ptr(), ctx.weight, up.data_ptr(),
              grad.data_ptr())
        return grad, None, None


def alpha_hole(alpha, mask, weight=1.0):
    """weight * mean over all H*W pixels of alpha * (1 - mask): the penalty on coverage in the target frame's holes; alpha
    [1,H,W] or [H,W] (the rasterizer's return_alpha output), mask as masked_l1_dssim's.  One HIP pass forward (per-workgroup
    partial sums, reduced in a fixed order in double: bit-repeatable) and one elementwise pass backward, weight * (1 - mask) /
    (H*W), bit-equal to torch autograd of the definition (lr_alpha_hole_forward / _backward)."""
    return _AlphaHole.apply(alpha, mask, weight)
