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

Frame: image float32 [H,W,3], mask / dilated / border uint8 [H,W], depth float32 [H,W], valid uint8 [N], pix int32 [N]
(valid and pix only for one pose), image_u8 uint8 [H,W,3].  mask is the reference's mask2 / maskj, dilated its round_mask2 after
the maximum filter, border its mask_hf, bit for bit; from valid and pix the caller gets, with torch indexing,
    valid_idx = valid.nonzero()[:, 0];  round_coord_cam2 = stack(pix[valid_idx] % W, pix[valid_idx] // W)
    border_valid_idx = border.flatten()[pix[valid_idx]].nonzero()[:, 0]
The IMAGE is this library's own definition, chosen by calling this module at all: a z-tested bilinear splat in fixed point
(include/lucid_raster.h), not griddata's Delaunay interpolation, which has no occlusion handling.  The reference's `edgemask`
patch (:400, :554) repairs griddata's hull edge and has no counterpart.  Everything is bit-repeatable (integer atomics only).

Device tensors only: a CPU tensor raises.  K, R, T are host values (numpy, lists or tensors), taken as float64.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

Frame = collections.namedtuple("Frame", "image mask dilated border depth valid pix image_u8")


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
