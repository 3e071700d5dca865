"""TSDF fusion of rendered depth and mesh extraction on the device (csrc/tsdf.hip, lr_tsdf_*).

The surface-reconstruction code bases whose regularisers this package renders (2DGS, RaDe-GS, PGSR: median depth, normals from
depth, distortion, the normal map) all end the same way: render depth along a trajectory, fuse the maps into a truncated signed
distance volume, extract a triangle mesh -- with Open3D on the host.  Here:

    TSDFVolume(origin, voxel_size, dims, trunc, device, max_weight=inf)      .tsdf / .weight / .color, .reset()
        .integrate(depth, K, R, T, color=None, pixel_weight=None, depth_max=inf)             one frame
        .integrate_batch(depths, K, Rs, Ts, colors=None, pixel_weights=None, depth_max=inf)  F frames, 8 per launch; equal, bit
                                                                                             for bit, to one frame at a time
        .extract_mesh(min_weight=1.0) -> (vertices [V,3] float32, colors [V,3] float32, faces [T,3] int32), device tensors
    pinhole_of(view) -> (K, R, T)     host float64 of a MiniCam / reference camera, the conventions of reproject.py
    fuse_views(volume, views, pc, opt, bg_color, depth="median" | "expected", alpha_min=0.5, render_fn=None)
    save_mesh_ply(path, vertices, colors, faces, normals=None)               binary little-endian, uchar colours

The definitions (include/lucid_raster.h) are this library's own, stated so that numpy reproduces them to the bit
(tests/tsdf_ref.py): samples at the lattice points origin + s (i, j, k), tensors [nz,ny,nx] with x fastest; the projection is
reproject's float64 one, pixel index = coordinate; a running weighted mean of min(1, (d - z) / trunc) per voxel; extraction over
the six Kuhn tetrahedra of every cell whose eight corners have weight >= min_weight, vertices welded per lattice edge, winding
from the combinatorics alone.  Nothing depends on an arrival order: two runs give the same bits.

Device tensors only: a CPU tensor raises.  K, R, T are host values (numpy, lists or tensors), taken as float64.  Inputs are
converted (float32 dtype refused, strides and 16-byte alignment made right by a copy), sizes and devices refused
(INTEGRATION.md 2o)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib

# frames per launch: csrc/common.h REPROJECT_FRAMES_PER_LAUNCH (tests/test_tsdf_cpu.py compares the two); fuse_views renders
# that many, then integrates.  Another value only changes the grouping, never the result.
FRAMES_PER_GROUP = 8


def _host64(m, shape, what):
    """Host float64 array of `shape` from a numpy array, a list or a tensor."""
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float64))
    if a.size != int(np.prod(shape)):
        raise ValueError(f"tsdf: {what} must hold {shape} values, got {a.shape}")
    return a.reshape(shape)


def _dense(t, shape, dev, what):
    """float32 device tensor of `shape` on `dev`, contiguous and 16-byte aligned: the tensor itself or a copy."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"tsdf: {what} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"tsdf: {what} must be on a HIP device (there is no CPU path)")
    if t.device != dev:
        raise ValueError(f"tsdf: {what} is on {t.device}, the volume on {dev}")
    if t.dtype != torch.float32:
        raise TypeError(f"tsdf: {what} must be float32, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"tsdf: {what} must be {tuple(shape)}, got {tuple(t.shape)}")
    t = t.detach().contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


class TSDFVolume:
    """A truncated signed distance volume on one device.  dims = (nx, ny, nz), every one >= 2 and 7 nx ny nz <= 2^31 - 2^12."""

    def __init__(self, origin, voxel_size, dims, trunc, device, max_weight=math.inf):
        self.origin = tuple(float(v) for v in origin)
        self.voxel_size = float(voxel_size)
        self.dims = tuple(int(v) for v in dims)
        self.trunc = float(trunc)
        self.max_weight = float(max_weight)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("tsdf.TSDFVolume: the volume lives on a HIP device (there is no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if len(self.origin) != 3 or len(self.dims) != 3:
            raise ValueError("tsdf.TSDFVolume: origin and dims hold three values each")
        nx, ny, nz = self.dims
        if min(self.dims) < 2 or 7 * nx * ny * nz > 2 ** 31 - 4096:
            raise ValueError(f"tsdf.TSDFVolume: dims must be >= 2 with 7 nx ny nz <= 2^31 - 2^12, got {self.dims}")
        if not (self.voxel_size > 0 and math.isfinite(self.voxel_size) and self.trunc > 0 and math.isfinite(self.trunc)):
            raise ValueError("tsdf.TSDFVolume: voxel_size and trunc must be finite and > 0")
        if not self.max_weight > 0:
            raise ValueError("tsdf.TSDFVolume: max_weight must be > 0")
        self.tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.color = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device=self.device)
        self.reset()

    def reset(self):
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        self.color.zero_()

    def _desc(self):
        nx, ny, nz = self.dims
        for name, t, shape in (("tsdf", self.tsdf, (nz, ny, nx)), ("weight", self.weight, (nz, ny, nx)),
                               ("color", self.color, (nz, ny, nx, 3))):
            # read and written in place: never copied
            if not (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == torch.float32 and
                    tuple(t.shape) == shape and t.is_contiguous() and t.data_ptr() % 16 == 0):
                raise ValueError(f"tsdf.TSDFVolume: .{name} must stay a contiguous, aligned float32 {shape} tensor on {self.device}")
        return _lib.TsdfVolumeDesc(origin=(ctypes.c_float * 3)(*self.origin), voxel_size=self.voxel_size, nx=nx, ny=ny, nz=nz,
                                   trunc=self.trunc, tsdf=self.tsdf.data_ptr(), weight=self.weight.data_ptr(),
                                   color=self.color.data_ptr())

    def integrate(self, depth, K, R, T, color=None, pixel_weight=None, depth_max=math.inf):
        """One frame: depth [H,W] float32, color [H,W,3], pixel_weight [H,W]; K 3x3, R 3x3, T 3 world to camera, host float64."""
        if not isinstance(depth, torch.Tensor) or depth.dim() != 2:
            raise ValueError("tsdf.integrate: depth must be a [H,W] tensor")
        return self.integrate_batch(depth[None], K, _host64(R, (1, 3, 3), "R"), _host64(T, (1, 3), "T"),
                                    colors=None if color is None else color[None],
                                    pixel_weights=None if pixel_weight is None else pixel_weight[None], depth_max=depth_max)

    def integrate_batch(self, depths, K, Rs, Ts, colors=None, pixel_weights=None, depth_max=math.inf):
        """F frames in index order: depths [F,H,W] float32, colors [F,H,W,3], pixel_weights [F,H,W]; Rs [F,3,3], Ts [F,3]."""
        if not isinstance(depths, torch.Tensor) or depths.dim() != 3:
            raise ValueError("tsdf.integrate_batch: depths must be a [F,H,W] tensor")
        F, H, W = (int(v) for v in depths.shape)
        if not 1 <= F <= 65535 or H < 2 or W < 2:
            raise ValueError(f"tsdf.integrate_batch: 1..65535 frames of H, W >= 2 required, got {F} of {H} x {W}")
        d = _dense(depths, (F, H, W), self.device, "depth")
        c = None if colors is None else _dense(colors, (F, H, W, 3), self.device, "color")
        pw = None if pixel_weights is None else _dense(pixel_weights, (F, H, W), self.device, "pixel_weight")
        Kh, Rh, Th = _host64(K, (3, 3), "K"), _host64(Rs, (F, 9), "Rs"), _host64(Ts, (F, 3), "Ts")
        args = _lib.TsdfIntegrateArgs(vol=self._desc(), n_frames=F, height=H, width=W, depth=d.data_ptr(),
                                      color=None if c is None else c.data_ptr(),
                                      pixel_weight=None if pw is None else pw.data_ptr(),
                                      K=Kh.ctypes.data, R=Rh.ctypes.data, T=Th.ctypes.data, depth_max=float(depth_max),
                                      max_weight=self.max_weight, stream=torch.cuda.current_stream(self.device).cuda_stream)
        with _lib.on_device(self.device):
            rc = _lib.lib().lr_tsdf_integrate(ctypes.byref(args))
        if rc < 0:
            _lib.raise_for(rc, "tsdf.integrate")
        return self

    def extract_mesh(self, min_weight=1.0):
        """(vertices [V,3] float32, colors [V,3] float32, faces [T,3] int32) on the volume's device; one host
        synchronisation (the two sizes).  An empty volume gives V = 0 and T = 0."""
        L = _lib.lib()
        dev = self.device
        nv, nf = ctypes.c_longlong(0), ctypes.c_longlong(0)
        args = _lib.TsdfExtractArgs(vol=self._desc(), min_weight=float(min_weight), out_n_vertices=ctypes.addressof(nv),
                                    out_n_faces=ctypes.addressof(nf), stream=torch.cuda.current_stream(dev).cuda_stream)
        ws_bytes = int(L.lr_tsdf_workspace_bytes(ctypes.byref(args)))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws_bytes
        with _lib.on_device(dev):
            rc = L.lr_tsdf_extract_count(ctypes.byref(args))
            if rc < 0:
                _lib.raise_for(rc, "tsdf.extract_mesh")
            V, T = int(nv.value), int(nf.value)
            vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
            colors = torch.empty((V, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((T, 3), dtype=torch.int32, device=dev)
            args.n_vertices, args.n_faces = V, T
            args.out_vertices = vertices.data_ptr() if V else None
            args.out_colors = colors.data_ptr() if V else None
            args.out_faces = faces.data_ptr() if T else None
            rc = L.lr_tsdf_extract_emit(ctypes.byref(args))
        if rc < 0:
            _lib.raise_for(rc, "tsdf.extract_mesh")
        return vertices, colors, faces


def pinhole_of(view):
    """(K [3,3], R [3,3], T [3]) host float64 of a camera with image_width, image_height, FoVx, FoVy and world_view_transform
    (cameras.MiniCam, the reference's Camera / MiniCam): fx = W / (2 tan(FoVx / 2)), fy likewise, cx = (W - 1) / 2,
    cy = (H - 1) / 2 (the pixel index is the coordinate, as in reproject), R = world_view_transform[:3,:3]^T,
    T = world_view_transform[3,:3]: p_cam = R x + T."""
    W, H = int(view.image_width), int(view.image_height)
    wvt = view.world_view_transform
    wvt = wvt.detach().cpu().numpy() if isinstance(wvt, torch.Tensor) else np.asarray(wvt)
    wvt = wvt.astype(np.float64)
    K = np.array([[W / (2.0 * math.tan(float(view.FoVx) / 2.0)), 0.0, (W - 1) / 2.0],
                  [0.0, H / (2.0 * math.tan(float(view.FoVy) / 2.0)), (H - 1) / 2.0],
                  [0.0, 0.0, 1.0]], dtype=np.float64)
    return K, np.ascontiguousarray(wvt[:3, :3].T), np.ascontiguousarray(wvt[3, :3])


def _view_depth_and_color(out, depth, alpha_min):
    """(depth [H,W], color [H,W,3]) of one render() result: median depth or the blended depth divided by alpha, 0 where
    alpha < alpha_min."""
    alpha = out["alpha"].detach()
    alpha = alpha.reshape(alpha.shape[-2], alpha.shape[-1])
    if depth == "median":
        d = out["median_depth"].detach().reshape(alpha.shape)
    else:
        d = out["depth"].detach().reshape(alpha.shape) / alpha
    d = torch.where(alpha < alpha_min, torch.zeros_like(d), d)
    return d.float().contiguous(), out["render"].detach().permute(1, 2, 0).float().contiguous()


def fuse_views(volume, views, pc, opt, bg_color, depth="median", alpha_min=0.5, render_fn=None):
    """Render every view (render_fn(view, pc, opt, bg_color, return_alpha=True, return_median=...), default
    gaussian_renderer.render) and integrate depth and colour into `volume`, FRAMES_PER_GROUP frames per launch, without a host
    copy.  depth: "median" (the depth at which the transmittance falls below one half) or "expected" (the blended depth divided
    by alpha); a pixel with alpha < alpha_min gets depth 0 and is skipped.  Equal, bit for bit, to rendering each view by hand
    and calling integrate() with pinhole_of(view).  All views of a group must share K (same size and field of view: a new group
    starts where they change).  Returns the volume."""
    if depth not in ("median", "expected"):
        raise ValueError(f"tsdf.fuse_views: depth must be 'median' or 'expected', got {depth!r}")
    if render_fn is None:
        from .gaussian_renderer import render as render_fn
    group = []

    def flush():
        if group:
            volume.integrate_batch(torch.stack([g[0] for g in group]), group[0][2], np.stack([g[3] for g in group]),
                                   np.stack([g[4] for g in group]), colors=torch.stack([g[1] for g in group]))
            group.clear()

    with torch.no_grad():
        for view in views:
            K, R, T = pinhole_of(view)
            out = render_fn(view, pc, opt, bg_color, return_alpha=True, return_median=depth == "median")
            d, c = _view_depth_and_color(out, depth, alpha_min)
            if group and (group[0][0].shape != d.shape or not np.array_equal(group[0][2], K)):
                flush()
            group.append((d, c, K, R, T))
            if len(group) == FRAMES_PER_GROUP:
                flush()
        flush()
    return volume


def save_mesh_ply(path, vertices, colors, faces, normals=None):
    """Binary little-endian PLY: float x y z, with `normals` float nx ny nz behind them, and uchar red green blue per vertex
    (colour clamped to [0,1], times 255, rounded half to even), one uchar count and three int indices per face.  Without
    normals the file is what it was before the argument existed."""
    v = vertices.detach().float().cpu().numpy().reshape(-1, 3)
    c = colors.detach().float().cpu().numpy().reshape(-1, 3)
    f = faces.detach().cpu().numpy().astype(np.int32).reshape(-1, 3)
    if c.shape != v.shape:
        raise ValueError(f"tsdf.save_mesh_ply: {v.shape[0]} vertices and {c.shape[0]} colours")
    c8 = np.rint(np.clip(np.nan_to_num(c, nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
    fields = [("xyz", "<f4", 3), ("rgb", "u1", 3)]
    if normals is not None:
        n = normals.detach().float().cpu().numpy().reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError(f"tsdf.save_mesh_ply: {v.shape[0]} vertices and {n.shape[0]} normals")
        fields.insert(1, ("nxyz", "<f4", 3))
    vrec = np.empty(v.shape[0], dtype=fields)
    vrec["xyz"], vrec["rgb"] = v, c8
    if normals is not None:
        vrec["nxyz"] = n
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", 3)])
    frec["n"], frec["idx"] = 3, f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n" +
              ("property float nx\nproperty float ny\nproperty float nz\n" if normals is not None else "") +
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
