"""Video frames on the device: the per-frame post-processing of LucidDreamer.render_video (R/luciddreamer.py:221-272) in HIP.

The reference renders every view, then forms the bytes of both videos on the host:
    frame: np.round(frame.permute(1,2,0).detach().cpu().numpy().clip(0,1)*255.).astype(np.uint8)
    depth: colorize(-(depth * (depth > 0)).detach().cpu().numpy())          (R/utils/depth.py: percentiles, jet, bytes)
Here both are HIP kernels (csrc/video.hip, lr_frames_to_u8 / lr_depth_colorize), byte for byte the same, and
iter_video_frames() pipelines the loop so that only the final uint8 bytes cross to the host, copied on a stream of their own.

    frames_to_uint8(images)               [3,H,W] or [N,3,H,W] float32 -> uint8 [...,H,W,3]  (device)
    colorize_depth(depth, ...)            [H,W], [1,H,W] or [N,1,H,W] float32 -> (uint8 [...,H,W,4], (vmin, vmax))  (device)
    jet_lut()                             matplotlib's jet LUT as bytes, [259, 4] uint8 (no matplotlib needed)
    iter_video_frames(views, pc, opt, bg) yields (frame_u8, depth_rgba) per view, in view order
    render_video_frames(...)              the two lists render_video hands to imageio.mimwrite

One difference from the reference, by design: a depth map without a valid pixel (every value == invalid_val) makes the
reference's np.percentile raise IndexError; colorize_depth returns the background colour everywhere and vmin = vmax = NaN.
"""
import collections

import numpy as np
import torch

from . import _lib

# matplotlib's jet colormap, its published segment data (x, y0, y1) per channel (matplotlib/_cm.py, _jet_data)
_JET_DATA = {
    "red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
    "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
    "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
}


def _lookup_table(N, data):
    """The piecewise-linear table of matplotlib.colors._create_lookup_table(N, data, gamma=1.0), in float64."""
    adata = np.array(data, dtype=np.float64)
    x, y0, y1 = adata[:, 0], adata[:, 1], adata[:, 2]
    if N == 1:
        lut = np.array(y0[-1])
    else:
        x = x * (N - 1)
        xind = (N - 1) * np.linspace(0, 1, N)
        ind = np.searchsorted(x, xind)[1:-1]
        distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut = np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
    return np.clip(lut, 0.0, 1.0)


def jet_lut(N=256):
    """matplotlib's jet `_lut` with N colours plus its under / over / bad rows, as colormap(..., bytes=True) uses it:
    uint8 [N + 3, 4] = (lut * 255).astype(uint8).  Under is colour 0, over colour N - 1, bad (0, 0, 0, 0)."""
    lut = np.ones((N + 3, 4), dtype=np.float64)
    for c, name in enumerate(("red", "green", "blue")):
        lut[:-3, c] = _lookup_table(N, _JET_DATA[name])
    lut[N] = lut[0]
    lut[N + 1] = lut[N - 1]
    lut[N + 2] = 0.0
    return (lut * 255).astype(np.uint8)


def _host_lut(cmap):
    """uint8 [N + 3, 4] LUT of `cmap`: 'jet' (built here), any other matplotlib colormap name or Colormap (needs matplotlib),
    or such a uint8 table itself."""
    if isinstance(cmap, str) and cmap == "jet":
        return jet_lut()
    if isinstance(cmap, np.ndarray):
        lut = cmap
    else:
        try:
            import matplotlib
        except ImportError as e:
            raise RuntimeError(f"colormap {cmap!r} needs matplotlib (only 'jet' is built in)") from e
        cm = matplotlib.colormaps[cmap] if isinstance(cmap, str) else cmap
        if not getattr(cm, "_isinit", True):
            cm._init()
        lut = (cm._lut * 255).astype(np.uint8)
    if lut.dtype != np.uint8 or lut.ndim != 2 or lut.shape[1] != 4 or not 4 <= lut.shape[0] <= 4096 + 3:
        raise ValueError(f"colormap LUT must be uint8 [N + 3, 4] with 1 <= N <= 4096, got {lut.dtype} {lut.shape}")
    return lut


_DEVICE_LUTS = {}                   # (device, key) -> (device tensor, N)


def _device_lut(cmap, dev):
    key = (str(dev), cmap if isinstance(cmap, str) else id(cmap))
    hit = _DEVICE_LUTS.get(key)
    if hit is None or not isinstance(cmap, str):
        lut = _host_lut(cmap)
        hit = (torch.from_numpy(np.ascontiguousarray(lut)).to(dev), lut.shape[0] - 3)
        if isinstance(cmap, str):
            _DEVICE_LUTS[key] = hit
    return hit


def _need_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"luciddreamer_amd.video.{what}: tensors must be on a HIP device (there is no CPU path)")


def frames_to_uint8(images):
    """uint8(rint(clamp(x, 0, 1) * 255)) in HWC order: [3,H,W] -> [H,W,3] or [N,3,H,W] -> [N,H,W,3], on the device.
    Byte for byte the reference's np.round(frame.permute(1,2,0).cpu().numpy().clip(0,1)*255.).astype(np.uint8)
    (float32, round half to even; NaN gives 0).  One launch for the whole batch, on the current stream."""
    if not isinstance(images, torch.Tensor):
        raise TypeError("frames_to_uint8: images must be a torch.Tensor")
    if images.dim() not in (3, 4) or images.shape[-3] != 3:
        raise ValueError(f"frames_to_uint8: images must be [3,H,W] or [N,3,H,W], got {tuple(images.shape)}")
    if images.dtype != torch.float32:
        raise TypeError(f"frames_to_uint8: images must be float32, got {images.dtype}")
    if images.numel() == 0:
        raise ValueError("frames_to_uint8: empty images")
    _need_device(images, "frames_to_uint8")
    x = images.detach().contiguous()
    n = 1 if x.dim() == 3 else int(x.shape[0])
    H, W = int(x.shape[-2]), int(x.shape[-1])
    out = torch.empty(tuple(x.shape[:-3]) + (H, W, 3), dtype=torch.uint8, device=x.device)
    L = _lib.lib()
    with _lib.on_device(x.device):
        rc = L.lr_frames_to_u8(n, H, W, x.data_ptr(), out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream)
    if rc < 0:
        _lib.raise_for(rc, "frames_to_uint8")
    return out


def _limit(v, n, dev):
    t = torch.as_tensor(v, dtype=torch.float32, device=dev).detach()
    if t.numel() not in (1, n):
        raise ValueError(f"colorize_depth: vmin / vmax must be a scalar or hold one value per frame ({n})")
    return t.reshape(-1).expand(n)


def colorize_depth(depth, vmin=None, vmax=None, cmap="jet", invalid_val=-99, invalid_mask=None,
                   background_color=(128, 128, 128, 255), gamma_corrected=False, value_transform=None, from_render=True):
    """R/utils/depth.py:colorize on the device, byte for byte, for a rendered depth map (from_render=True: the value is
    -(depth * (depth > 0)), what render_video hands to colorize) or for the value itself (from_render=False).

    depth: float32 [H,W] or [1,H,W] (one frame -> uint8 [H,W,4]) or [N,1,H,W] (a batch -> [N,H,W,4], same launches).
    vmin / vmax: None = the 2nd / 98th percentile of the valid pixels (np.percentile in float32, selected on the device without
    a sort), or fixed limits (numbers or tensors, scalar or one per frame; taken as float32).
    cmap: 'jet' (built in), or any matplotlib colormap name / Colormap when matplotlib is importable.
    Returns (rgba, (vmin, vmax)): device tensors; vmin / vmax are float32 of shape [] or [N].  No host synchronisation.
    A frame without a valid pixel (the reference raises IndexError) is all background with vmin = vmax = NaN."""
    if invalid_mask is not None or gamma_corrected or value_transform is not None:
        raise NotImplementedError("colorize_depth: invalid_mask, gamma_corrected and value_transform are not supported")
    if not isinstance(depth, torch.Tensor):
        raise TypeError("colorize_depth: depth must be a torch.Tensor")
    if depth.dim() == 2:
        lead, n = (), 1
    elif depth.dim() == 3 and depth.shape[0] == 1:
        lead, n = (), 1
    elif depth.dim() == 4 and depth.shape[1] == 1:
        lead, n = (int(depth.shape[0]),), int(depth.shape[0])
    else:
        raise ValueError(f"colorize_depth: depth must be [H,W], [1,H,W] or [N,1,H,W], got {tuple(depth.shape)}")
    if depth.dtype != torch.float32:
        raise TypeError(f"colorize_depth: depth must be float32, got {depth.dtype}")
    if depth.numel() == 0:
        raise ValueError("colorize_depth: empty depth")
    bg = bytes(int(c) for c in background_color)             # raises on values outside 0..255
    if len(bg) != 4:
        raise ValueError("colorize_depth: background_color must be 4 values (RGBA)")
    _need_device(depth, "colorize_depth")
    dev = depth.device
    d = depth.detach().contiguous()
    H, W = int(d.shape[-2]), int(d.shape[-1])
    lut, lut_n = _device_lut(cmap, dev)
    fixed = None
    if vmin is not None and vmax is not None:
        fixed = torch.stack([_limit(vmin, n, dev), _limit(vmax, n, dev)], dim=1).contiguous()
    L = _lib.lib()
    out = torch.empty(lead + (H, W, 4), dtype=torch.uint8, device=dev)
    vmm = torch.empty((n, 2), dtype=torch.float32, device=dev)
    ws_bytes = int(L.lr_video_workspace_bytes(n, H, W))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) if fixed is None else None
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run(fixed_t):
        with _lib.on_device(dev):
            rc = L.lr_depth_colorize(n, H, W, d.data_ptr(), 1 if from_render else 0, float(invalid_val), 2.0, 98.0,
                                     fixed_t.data_ptr() if fixed_t is not None else None, lut.data_ptr(), lut_n, bg,
                                     out.data_ptr(), vmm.data_ptr(), ws.data_ptr() if ws is not None else None,
                                     ws_bytes if ws is not None else 0, stream)
        if rc < 0:
            _lib.raise_for(rc, "colorize_depth")

    run(fixed)
    if fixed is None and (vmin is not None or vmax is not None):
        # one limit given: the other is the percentile, as in the reference; colour again with both fixed
        lo = _limit(vmin, n, dev) if vmin is not None else vmm[:, 0]
        hi = _limit(vmax, n, dev) if vmax is not None else vmm[:, 1]
        run(torch.stack([lo, hi], dim=1).contiguous())
    lims = vmm[0] if not lead else vmm.t()
    return out, (lims[0], lims[1])


def iter_video_frames(views, pc, opt, bg_color, *, depth=True, in_flight=8, to_host=True, render_fn=None):
    """The loop of render_video (R/luciddreamer.py:250-255) with its post-processing on the device.  Yields
    (frame_u8 [H,W,3], depth_rgba [H,W,4] or None when depth=False) per view, in view order.
    depth="median" colourises the median depth instead of the expected one (no smear between foreground and background at object
    edges): the view is rendered with return_median=True, which `render_fn` must then accept (gaussian_renderer.render and
    render_raw do), and out["median_depth"] goes to colorize_depth.

    Each view runs `render_fn(view, pc, opt, bg_color)` (default: gaussian_renderer.render, the forward the drop-in takes;
    pass gaussian_renderer.render_raw or the caller's own render) under torch.no_grad(), then frames_to_uint8 and
    colorize_depth on the caller's stream.  With to_host=True the uint8 results go to the host on a copy stream of their own,
    into `in_flight` pinned slots guarded by events: the host waits only when it yields a frame or reuses a slot, and the
    yielded numpy arrays are the caller's own (copied out of the slot).  With to_host=False the device tensors are yielded.
    The global configuration (luciddreamer_amd.config) is not touched."""
    if depth not in (True, False, "median"):
        raise ValueError('iter_video_frames: depth must be True, False or "median"')
    in_flight = int(in_flight)
    if in_flight < 1:
        raise ValueError("iter_video_frames: in_flight must be >= 1")
    xyz = pc._xyz if hasattr(pc, "_xyz") else pc.get_xyz
    _need_device(xyz, "iter_video_frames")
    if render_fn is None:
        from .gaussian_renderer import render as render_fn
    dev = xyz.device
    return _frames(views, pc, opt, bg_color, depth, in_flight, to_host, render_fn, dev)


def _frames(views, pc, opt, bg_color, depth, in_flight, to_host, render_fn, dev):
    compute = torch.cuda.current_stream(dev)
    copy = torch.cuda.Stream(device=dev) if to_host else None
    slots = [None] * in_flight
    pending = collections.deque()

    def take(slot):
        slot["event"].synchronize()
        f = slot["frame"].numpy().copy()
        return f, (slot["depth"].numpy().copy() if slot["depth"] is not None else None)

    try:
        for i, view in enumerate(views):
            with torch.no_grad():
                median = isinstance(depth, str)             # "median" (iter_video_frames checked it)
                out = render_fn(view, pc, opt, bg_color, return_median=True) if median else render_fn(view, pc, opt, bg_color)
                f = frames_to_uint8(out["render"])
                c = colorize_depth(out["median_depth" if median else "depth"])[0] if depth else None
            if not to_host:
                yield f, c
                continue
            if len(pending) == in_flight:
                yield take(pending.popleft())
            k = i % in_flight
            slot = slots[k]
            if slot is None or slot["frame"].shape != f.shape or (c is not None and slot["depth"].shape != c.shape):
                slot = slots[k] = {"frame": torch.empty(f.shape, dtype=torch.uint8, pin_memory=True),
                                   "depth": torch.empty(c.shape, dtype=torch.uint8, pin_memory=True) if c is not None else None,
                                   "event": torch.cuda.Event()}
            copy.wait_stream(compute)
            with torch.cuda.stream(copy):
                slot["frame"].copy_(f, non_blocking=True)
                f.record_stream(copy)
                if c is not None:
                    slot["depth"].copy_(c, non_blocking=True)
                    c.record_stream(copy)
                slot["event"].record(copy)
            pending.append(slot)
        while pending:
            yield take(pending.popleft())
    finally:
        if copy is not None and pending:
            copy.synchronize()              # a consumer that stopped early: no copy into a freed slot


def render_video_frames(views, pc, opt, bg_color, **kwargs):
    """(framelist, depthlist): the two lists render_video hands to imageio.mimwrite, host uint8 arrays [H,W,3] / [H,W,4]
    (depthlist empty with depth=False).  Keyword arguments as iter_video_frames."""
    frames, depths = [], []
    for f, d in iter_video_frames(views, pc, opt, bg_color, **kwargs):
        frames.append(f)
        if d is not None:
            depths.append(d)
    return frames, depths
