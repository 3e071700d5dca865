"""Point-cloud reprojection on the device: the warped frames and hole masks of LucidDreamer.generate_pcd
(R/luciddreamer.py:382-413 "Dreaming", :516-570 "Aligning") in HIP (csrc/reproject.hip, lr_reproject / lr_lift).

The reference projects the whole accumulated cloud into every new pose on the host, interpolates an image with
scipy.interpolate.griddata and forms the hole mask with a 9x9 maximum and an 11x11 minimum filter; "Aligning" does it again
for 5 hemisphere poses per dream pose.  Here:

    lift(depth, K, R, T)                               [H,W] float32 -> world points [3, H*W] float32    (:370-371, :451-453)
    project(points, colors, K, R, T, H, W)             one pose  -> Frame
    project_batch(points, colors, K, Rs, Ts, H, W)     F poses of one cloud in the same launches -> Frame with a leading F
    align_frames(points, colors, K, render_poses, inner_poses, H, W, fov_x)   the reference's `traindata` dict (:498-505, :567-570)
    compose_pose / pc2w                                the pose algebra of :527-534 on the host, float64
and, once the networks have produced the new view's image and depth map (:424-493; csrc/dream.hip, lr_dream_*):
    fit_scale(points, frame, depth, K, R, T)           the scale of the depth map against the cloud, in closed form -> ScaleFit
    scatter_interpolate(uv, values, H, W, where)       scattered samples into the pixels whose `where` byte is 0 -> [H,W] float32
    compensate(points, frame, depth, K, R, T, scale)   border correspondences, their offsets interpolated into the holes,
                                                       the corrected depth lifted -> Compensation
    dream_step(points, colors, frame, image, depth, K, R, T, scale="lstsq")   all of it and the append -> (points', colors', info)

Frame: image float32 [H,W,3], mask / dilated / border uint8 [H,W], depth float32 [H,W], valid uint8 [N], pix int32 [N]
(valid and pix only for one pose), image_u8 uint8 [H,W,3].  mask is the reference's mask2 / maskj, dilated its round_mask2 after
the maximum filter, border its mask_hf, bit for bit; from valid and pix the caller gets, with torch indexing,
    valid_idx = valid.nonzero()[:, 0];  round_coord_cam2 = stack(pix[valid_idx] % W, pix[valid_idx] // W)
    border_valid_idx = border.flatten()[pix[valid_idx]].nonzero()[:, 0]
The IMAGE is this library's own definition, chosen by calling this module at all: a z-tested bilinear splat in fixed point
(include/lucid_raster.h), not griddata's Delaunay interpolation, which has no occlusion handling.  The reference's `edgemask`
patch (:400, :554) repairs griddata's hull edge and has no counterpart.  Everything is bit-repeatable (integer atomics only).

What is OURS in the second group: the interpolation (a moving least squares fit of an affine function with inverse-distance
weights, clamped to the samples' range; include/lucid_raster.h), not griddata's Delaunay triangulation; the scale in closed form
(Spq / Sqq), where the reference runs 100 Adam steps that never move its scale from 1 (scale="reference"); float64 throughout.

Device tensors only: a CPU tensor raises.  K, R, T are host values (numpy, lists or tensors), taken as float64.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

Frame = collections.namedtuple("Frame", "image mask dilated border depth valid pix image_u8")
ScaleFit = collections.namedtuple("ScaleFit", "scale n_used spp spq sqq mse_before mse_after")
Compensation = collections.namedtuple("Compensation", "new_depth lifted n_corr corr_uv corr_value")
DreamInfo = collections.namedtuple("DreamInfo", "fit scale n_corr n_added")
SCATTER_TILE = _lib.LR_SCATTER_TILE                  # samples per on-chip tile of scatter_interpolate


def _need_device(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"luciddreamer_amd.reproject.{what}: expected a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"luciddreamer_amd.reproject.{what}: tensors must be on a HIP device (there is no CPU path)")


def _host64(m, shape, what):
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float64))
    if a.size != int(np.prod(shape)):
        raise ValueError(f"reproject: {what} must hold {shape} values, got {a.shape}")
    return a.reshape(shape)


def _points(points, what):
    _need_device(points, what)
    if points.dtype != torch.float32:
        raise TypeError(f"reproject.{what}: points must be float32, got {points.dtype}")
    if points.dim() != 2 or 3 not in points.shape:
        raise ValueError(f"reproject.{what}: points must be [N,3] or [3,N], got {tuple(points.shape)}")
    p = points.detach().contiguous()
    if p.shape[1] == 3:                                      # a 3 x 3 tensor is read as [N,3]
        return p, int(p.shape[0]), 3, 1
    return p, int(p.shape[1]), 1, int(p.shape[1])


def compose_pose(Ri2j, Ti2j, Rw2i, Tw2i):
    """World-to-camera of inner pose j seen from render pose i (R/luciddreamer.py:527-528), float64 on the host."""
    Rw2j = np.matmul(Ri2j, Rw2i)
    Tw2j = np.matmul(Ri2j, Tw2i) + Ti2j
    return Rw2j, Tw2j


def pc2w(Rw2j, Tw2j):
    """The `transform_matrix` of a frame: camera to world with the y and z axes reversed (R/luciddreamer.py:531-534)."""
    yz_reverse = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]])
    Rj2w = np.matmul(yz_reverse, Rw2j).T
    Tj2w = -np.matmul(Rj2w, np.matmul(yz_reverse, Tw2j))
    P = np.concatenate((Rj2w, Tj2w), axis=1)
    return np.concatenate((P, np.array([[0, 0, 0, 1]])), axis=0)


def lift(depth, K, R, T):
    """World points [3, H*W] float32 of a depth map [H,W] seen from the world-to-camera pose (R, T):
    inv(R) (inv(K) (x d, y d, d)) - inv(R) T in float64 on the device; the inverses are formed here on the host."""
    _need_device(depth, "lift")
    if depth.dtype != torch.float32 or depth.dim() != 2 or depth.numel() == 0:
        raise ValueError(f"reproject.lift: depth must be a non-empty float32 [H,W], got {depth.dtype} {tuple(depth.shape)}")
    d = depth.detach().contiguous()
    H, W = int(d.shape[0]), int(d.shape[1])
    Kinv = np.ascontiguousarray(np.linalg.inv(_host64(K, (3, 3), "K")))
    Rinv = np.ascontiguousarray(np.linalg.inv(_host64(R, (3, 3), "R")))
    t = _host64(T, (3,), "T")
    RinvT = np.array([(Rinv[i, 0] * t[0] + Rinv[i, 1] * t[1]) + Rinv[i, 2] * t[2] for i in range(3)], dtype=np.float64)
    out = torch.empty((3, H * W), dtype=torch.float32, device=d.device)
    L = _lib.lib()
    with _lib.on_device(d.device):
        rc = L.lr_lift(H, W, d.data_ptr(), Kinv.ctypes.data, Rinv.ctypes.data, RinvT.ctypes.data, out.data_ptr(),
                       torch.cuda.current_stream(d.device).cuda_stream)
    if rc < 0:
        _lib.raise_for(rc, "reproject.lift")
    return out


def _run(points, colors, K, Rs, Ts, H, W, z_tolerance, single, image, what):
    p, N, ps, cs = _points(points, what)
    dev = p.device
    c = None
    if image:
        _need_device(colors, what)
        if colors.dtype != torch.float32 or tuple(colors.shape) != (N, 3):
            raise ValueError(f"reproject.{what}: colors must be float32 [{N},3], got {colors.dtype} {tuple(colors.shape)}")
        if colors.device != dev:
            raise ValueError(f"reproject.{what}: points and colors are on different devices")
        c = colors.detach().contiguous()
    H, W = int(H), int(W)
    Kh = _host64(K, (3, 3), "K")
    F = int(Rs.shape[0])
    if F < 1:
        raise ValueError(f"reproject.{what}: at least one pose is required")
    L = _lib.lib()
    ws_bytes = int(L.lr_reproject_workspace_bytes(F, H, W))
    if ws_bytes == 0:
        raise ValueError(f"reproject.{what}: 1..65535 poses and H, W >= 2 required, got {F} poses of {H} x {W}")
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    img, img8 = (f32(F, H, W, 3), u8(F, H, W, 3)) if image else (None, None)
    mask, dil, border, depth = u8(F, H, W), u8(F, H, W), u8(F, H, W), f32(F, H, W)
    valid = u8(N) if single else None
    pix = torch.empty((N,), dtype=torch.int32, device=dev) if single else None
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None
    args = _lib.ReprojectArgs(n_points=N, points=ptr(p), point_stride=ps, coord_stride=cs, colors=ptr(c), n_frames=F, height=H,
                              width=W, z_tolerance=float(z_tolerance), K=Kh.ctypes.data, R=Rs.ctypes.data, T=Ts.ctypes.data,
                              out_image=ptr(img), out_image_u8=ptr(img8), out_mask=ptr(mask), out_dilated=ptr(dil),
                              out_border=ptr(border), out_depth=ptr(depth), out_valid=ptr(valid), out_pix=ptr(pix),
                              workspace=ws.data_ptr(), workspace_bytes=ws_bytes,
                              stream=torch.cuda.current_stream(dev).cuda_stream)
    with _lib.on_device(dev):
        rc = L.lr_reproject(ctypes.byref(args))
    if rc < 0:
        _lib.raise_for(rc, f"reproject.{what}")
    out = Frame(img, mask, dil, border, depth, valid, pix, img8)
    if single:
        out = Frame(*[t[0] if t is not None and k not in ("valid", "pix") else t for k, t in zip(Frame._fields, out)])
    return out


def project(points, colors, K, R, T, H, W, *, z_tolerance=0.05, image=True):
    """The cloud seen from one world-to-camera pose (R 3x3, T 3x1; K 3x3; host float64): a Frame.  image=False skips the
    splat (mask, dilated, border, depth, valid and pix only; colors may then be None)."""
    Rs = _host64(R, (1, 9), "R")
    Ts = _host64(T, (1, 3), "T")
    return _run(points, colors, K, Rs, Ts, H, W, z_tolerance, True, image, "project")


def project_batch(points, colors, K, Rs, Ts, H, W, *, z_tolerance=0.05, image=True):
    """F poses of one cloud in the same launches (Rs [F,3,3], Ts [F,3] or [F,3,1]): a Frame whose tensors carry a leading F;
    valid and pix are None.  Equal, bit for bit, to F calls of project()."""
    Rs = np.asarray(Rs.detach().cpu().numpy() if isinstance(Rs, torch.Tensor) else Rs, dtype=np.float64)
    F = int(Rs.shape[0]) if Rs.ndim == 3 else 0
    return _run(points, colors, K, _host64(Rs, (F, 9), "Rs"), _host64(Ts, (F, 3), "Ts"), H, W, z_tolerance, False, image,
                "project_batch")


def align_frames(points, colors, K, render_poses, inner_poses, H, W, fov_x, *, z_tolerance=0.05, as_tensors=False):
    """The "Aligning" loop of generate_pcd (R/luciddreamer.py:497-570): every render pose i ([n,>=3,4] world to camera) composed
    with every inner pose j, the cloud projected into each, one project_batch per render pose.  Returns the reference's traindata:
    {camera_angle_x, W, H, pcd_points [3,N], pcd_colors [N,3], frames: [{image, transform_matrix}]}, frames in (i, j) order; a pose
    that sees no point is skipped (:544).  Images are PIL.Image (as_tensors=False; pcd_points / pcd_colors numpy, as the reference
    holds them) or device uint8 [H,W,3] tensors (as_tensors=True; the cloud stays the caller's device tensors).  One host
    synchronisation per render pose (which poses saw a point)."""
    p, N, ps, _ = _points(points, "align_frames")
    _need_device(colors, "align_frames")
    rp = np.asarray(render_poses.detach().cpu().numpy() if isinstance(render_poses, torch.Tensor) else render_poses, dtype=np.float64)
    ip = np.asarray(inner_poses.detach().cpu().numpy() if isinstance(inner_poses, torch.Tensor) else inner_poses, dtype=np.float64)
    if rp.ndim != 3 or ip.ndim != 3 or rp.shape[1] < 3 or ip.shape[1] < 3 or rp.shape[2] != 4 or ip.shape[2] != 4:
        raise ValueError("reproject.align_frames: render_poses and inner_poses must be [n,3,4] or [n,4,4]")
    pts3n = p.t() if ps == 3 else p
    data = {"camera_angle_x": fov_x, "W": int(W), "H": int(H),
            "pcd_points": pts3n if as_tensors else pts3n.cpu().numpy(),
            "pcd_colors": colors if as_tensors else colors.detach().cpu().numpy(),
            "frames": []}
    if not as_tensors:
        from PIL import Image
    for i in range(rp.shape[0]):
        poses = [compose_pose(ip[j, :3, :3], ip[j, :3, 3:4], rp[i, :3, :3], rp[i, :3, 3:4]) for j in range(ip.shape[0])]
        if not poses:
            continue
        fr = project_batch(p, colors, K, np.stack([r for r, _ in poses]), np.stack([t for _, t in poses]), H, W,
                           z_tolerance=z_tolerance)
        seen = fr.dilated.flatten(1).any(dim=1).cpu().numpy()       # a valid point <=> a hit pixel <=> a dilated pixel
        host = None if as_tensors else fr.image_u8.cpu().numpy()
        for j, (Rw2j, Tw2j) in enumerate(poses):
            if not seen[j]:
                continue
            img = fr.image_u8[j] if as_tensors else Image.fromarray(host[j])
            data["frames"].append({"image": img, "transform_matrix": pc2w(Rw2j, Tw2j).tolist()})
    return data


# ---- dreaming: what follows the networks (R/luciddreamer.py:424-493) --------------------------------------------------------------
def scale_fit_from_sums(spp, spq, sqq, n):
    """The closed-form minimiser of the reference's loss mean |P - s q|^2 (:436) from its three sums: scale = spq / sqq,
    mse(s) = (spp - 2 s spq + s^2 sqq) / (3 n).  No usable pair, or sqq == 0, gives scale 1."""
    spp, spq, sqq, n = float(spp), float(spq), float(sqq), int(n)
    scale = spq / sqq if n > 0 and sqq != 0.0 else 1.0
    mse = (lambda s: (spp - 2.0 * s * spq + s * s * sqq) / (3.0 * n)) if n > 0 else (lambda s: 0.0)
    return ScaleFit(scale, n, spp, spq, sqq, mse(1.0), mse(scale))


def _one_pose(frame, depth, what):
    """The Frame of ONE pose (valid and pix present) and a depth map of its size; a device tensor each."""
    if not isinstance(frame, Frame):
        raise TypeError(f"reproject.{what}: frame must be a reproject.Frame")
    if frame.valid is None or frame.pix is None or frame.mask is None or frame.mask.dim() != 2:
        raise ValueError(f"reproject.{what}: needs the Frame of one pose (project(), with valid and pix), not a batch")
    _need_device(depth, what)
    _need_device(frame.mask, what)
    H, W = int(frame.mask.shape[0]), int(frame.mask.shape[1])
    if depth.dtype != torch.float32 or tuple(depth.shape) != (H, W):
        raise ValueError(f"reproject.{what}: depth must be float32 [{H},{W}] (the frame's size), got {depth.dtype} "
                         f"{tuple(depth.shape)}")
    if depth.device != frame.mask.device:
        raise ValueError(f"reproject.{what}: depth and frame are on different devices")
    return depth.detach().contiguous(), H, W


def _cloud_of(points, frame, what):
    p, N, ps, cs = _points(points, what)
    if int(frame.valid.numel()) != N or int(frame.pix.numel()) != N:
        raise ValueError(f"reproject.{what}: the frame was projected from {int(frame.valid.numel())} points, the cloud has {N}")
    if p.device != frame.mask.device:
        raise ValueError(f"reproject.{what}: points and frame are on different devices")
    return p, N, ps, cs


class _Pose:
    """K, R, T and the inverses lift() forms, host float64, kept alive for the C call."""
    def __init__(self, K, R, T):
        self.K = _host64(K, (3, 3), "K")
        self.R = _host64(R, (3, 3), "R")
        self.T = _host64(T, (3,), "T")
        self.Kinv = np.ascontiguousarray(np.linalg.inv(self.K))
        self.Rinv = np.ascontiguousarray(np.linalg.inv(self.R))
        t = self.T
        self.RinvT = np.array([(self.Rinv[i, 0] * t[0] + self.Rinv[i, 1] * t[1]) + self.Rinv[i, 2] * t[2] for i in range(3)],
                              dtype=np.float64)

    def fields(self):
        return dict(K=self.K.ctypes.data, R=self.R.ctypes.data, T=self.T.ctypes.data, Kinv=self.Kinv.ctypes.data,
                    Rinv=self.Rinv.ctypes.data, RinvT=self.RinvT.ctypes.data)


def _call(fn, args, dev, what):
    with _lib.on_device(dev):
        rc = fn(ctypes.byref(args))
    if rc < 0:
        _lib.raise_for(rc, f"reproject.{what}")


def fit_scale(points, frame, depth, K, R, T):
    """The scale s that brings the new view's depth map onto the cloud (:424-440): over every valid point P and the lift q of
    the depth under its pixel, s = sum P.q / sum q.q minimises the reference's loss mean |P - s q|^2.  One launch pair and one
    32-byte read-back.  Returns ScaleFit(scale, n_used, spp, spq, sqq, mse_before, mse_after): mse at s = 1 and at the fit."""
    d, H, W = _one_pose(frame, depth, "fit_scale")
    p, N, ps, cs = _cloud_of(points, frame, "fit_scale")
    dev = d.device
    pose = _Pose(K, R, T)
    L = _lib.lib()
    out = torch.empty((4,), dtype=torch.float64, device=dev)           # Spp, Spq, Sqq and the count's 8 bytes
    ws_bytes = int(L.lr_dream_workspace_bytes(N))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    valid, pix = frame.valid.contiguous(), frame.pix.contiguous()
    ptr = lambda t: t.data_ptr() if t.numel() > 0 else None
    args = _lib.DreamArgs(n_points=N, points=ptr(p), point_stride=ps, coord_stride=cs, valid=ptr(valid), pix=ptr(pix), height=H,
                          width=W, depth=d.data_ptr(), out_sums=out.data_ptr(), out_count=out.data_ptr() + 24,
                          workspace=ws.data_ptr(), workspace_bytes=ws_bytes, stream=torch.cuda.current_stream(dev).cuda_stream,
                          **pose.fields())
    _call(L.lr_dream_scale_sums, args, dev, "fit_scale")
    host = out.cpu()
    return scale_fit_from_sums(host[0], host[1], host[2], int(host[3:4].view(torch.int64)[0]))


def _scatter(su, sv, sval, M, H, W, where, what):
    dev = where.device
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    ptr = lambda t: t.data_ptr() if M > 0 else None
    args = _lib.ScatterArgs(n_samples=M, su=ptr(su), sv=ptr(sv), sval=ptr(sval), height=H, width=W, where=where.data_ptr(),
                            out=out.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    _call(_lib.lib().lr_scatter_interpolate, args, dev, what)
    return out


def scatter_interpolate(uv, values, H, W, where):
    """Scattered samples interpolated into the pixels of an H x W image whose `where` byte is 0 (uint8 or bool [H,W]); 0
    elsewhere and where no sample is usable.  uv [M,2] float64 (column, row), values [M] float64, M >= 0; a NaN value is
    skipped.  A moving least squares fit of an affine function with weights 1 / (d^2 + 1e-12)^2, clamped to the samples' range
    (formulas: include/lucid_raster.h).  float32 [H,W], bit-repeatable."""
    _need_device(uv, "scatter_interpolate")
    _need_device(values, "scatter_interpolate")
    _need_device(where, "scatter_interpolate")
    H, W = int(H), int(W)
    if uv.dtype != torch.float64 or uv.dim() != 2 or uv.shape[1] != 2:
        raise ValueError(f"reproject.scatter_interpolate: uv must be float64 [M,2], got {uv.dtype} {tuple(uv.shape)}")
    M = int(uv.shape[0])
    if values.dtype != torch.float64 or tuple(values.shape) != (M,):
        raise ValueError(f"reproject.scatter_interpolate: values must be float64 [{M}], got {values.dtype} {tuple(values.shape)}")
    if where.dtype not in (torch.uint8, torch.bool) or tuple(where.shape) != (H, W):
        raise ValueError(f"reproject.scatter_interpolate: where must be uint8 or bool [{H},{W}], got {where.dtype} "
                         f"{tuple(where.shape)}")
    if uv.device != where.device or values.device != where.device:
        raise ValueError("reproject.scatter_interpolate: uv, values and where are on different devices")
    w8 = where.detach().contiguous()
    w8 = w8.view(torch.uint8) if w8.dtype == torch.bool else w8
    uvt = uv.detach().t().contiguous()                                 # [2, M]: a plane each
    return _scatter(uvt[0], uvt[1], values.detach().contiguous(), M, H, W, w8, "scatter_interpolate")


def compensate(points, frame, depth, K, R, T, scale=1.0):
    """The depth compensation of :443-489.  The cloud points on the hole's border (border_valid_idx of :414, one nonzero and with
    it one host synchronisation) give, each, how far along its camera ray the scaled new depth is from the cloud; that offset is
    interpolated into every hole pixel (frame.mask == 0; the four image corners count as samples of 0) and the corrected depth
    is lifted.  Returns Compensation(new_depth [H,W] float32, 0 inside the mask; lifted [3, H*W] float32 = scale * lift(depth +
    new_depth); n_corr; corr_uv [n_corr + 4, 2] and corr_value [n_corr + 4] float64, the samples with the corners last)."""
    d, H, W = _one_pose(frame, depth, "compensate")
    p, N, ps, cs = _cloud_of(points, frame, "compensate")
    dev = d.device
    scale = float(scale)
    pose = _Pose(K, R, T)
    L = _lib.lib()
    valid, pix = frame.valid.contiguous(), frame.pix.contiguous()
    # valid_idx[border_valid_idx] of INTEGRATION.md 2j in one nonzero: a valid point whose pixel is on the border
    on_border = frame.border.reshape(-1)[pix.clamp(min=0).long()].bool() & valid.bool()
    corr = on_border.nonzero()[:, 0].to(torch.int32).contiguous()
    M = int(corr.numel())
    s3 = torch.empty((3, M + 4), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: t.data_ptr() if t.numel() > 0 else None
    common = dict(height=H, width=W, depth=d.data_ptr(), scale=scale, stream=stream, **pose.fields())
    args = _lib.DreamArgs(n_points=N, points=ptr(p), point_stride=ps, coord_stride=cs, pix=ptr(pix), corr=ptr(corr), n_corr=M,
                          out_su=s3[0].data_ptr(), out_sv=s3[1].data_ptr(), out_sval=s3[2].data_ptr(), **common)
    _call(L.lr_dream_correspond, args, dev, "compensate")
    new_depth = _scatter(s3[0], s3[1], s3[2], M + 4, H, W, frame.mask.contiguous(), "compensate")
    lifted = torch.empty((3, H * W), dtype=torch.float32, device=dev)
    args = _lib.DreamArgs(new_depth=new_depth.data_ptr(), out_points=lifted.data_ptr(), **common)
    _call(L.lr_dream_lift, args, dev, "compensate")
    return Compensation(new_depth, lifted, M, s3[:2].t(), s3[2])


_U8_TO_UNIT = np.arange(256, dtype=np.float32) / np.float32(255.0)    # the reference's astype(float32) / 255. (:490), exactly


def dream_step(points, colors, frame, image, depth, K, R, T, scale="lstsq"):
    """One dream pose after its networks (:424-493): align the new view's depth map to the cloud, compensate it inside the holes
    and append the hole pixels, the cloud never leaving the device.  frame = project(points, colors, K, R, T, H, W); image is the
    inpainted view, uint8 [H,W,3] (divided by 255) or float32 [H,W,3] (as is); depth float32 [H,W].
    scale: "lstsq" (fit_scale's closed form), "reference" (1.0 and no launch: what the reference's Adam fit yields, its scale
    never receiving a gradient) or a float.
    Returns (points' [3, N + n], colors' [N + n, 3], DreamInfo(fit, scale, n_corr, n_added)): the hole pixels (frame.mask == 0)
    in row-major order behind the cloud, positions from the compensated lift.  points may be [N,3] or [3,N]."""
    d, H, W = _one_pose(frame, depth, "dream_step")
    p, N, ps, _ = _cloud_of(points, frame, "dream_step")
    _need_device(colors, "dream_step")
    _need_device(image, "dream_step")
    if colors.dtype != torch.float32 or tuple(colors.shape) != (N, 3):
        raise ValueError(f"reproject.dream_step: colors must be float32 [{N},3], got {colors.dtype} {tuple(colors.shape)}")
    if image.dtype not in (torch.uint8, torch.float32) or tuple(image.shape) != (H, W, 3):
        raise ValueError(f"reproject.dream_step: image must be uint8 or float32 [{H},{W},3], got {image.dtype} "
                         f"{tuple(image.shape)}")
    fit = None
    if isinstance(scale, str):
        if scale == "lstsq":
            fit = fit_scale(p, frame, d, K, R, T)
            s = fit.scale
        elif scale == "reference":
            s = 1.0
        else:
            raise ValueError(f"reproject.dream_step: scale must be 'lstsq', 'reference' or a number, got {scale!r}")
    else:
        s = float(scale)
    comp = compensate(p, frame, d, K, R, T, scale=s)
    hole = (frame.mask.reshape(-1) == 0).nonzero()[:, 0]               # row-major, as np.where (:451, :490)
    new_points = comp.lifted[:, hole]
    if image.dtype == torch.uint8:
        lut = torch.from_numpy(_U8_TO_UNIT).to(image.device)
        new_colors = lut[image.reshape(-1, 3)[hole].long()]
    else:
        new_colors = image.reshape(-1, 3)[hole]
    pts3n = p.t() if ps == 3 else p
    return (torch.cat([pts3n, new_points], dim=1).contiguous(), torch.cat([colors.detach(), new_colors], dim=0).contiguous(),
            DreamInfo(fit, s, comp.n_corr, int(hole.numel())))
