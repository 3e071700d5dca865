"""A triangle mesh out of a Gaussian scene, on the device: render depth along a trajectory, fuse it into a TSDF volume, extract.

    python examples/extract_mesh.py [--points 400000] [--size 256] [--views 30] [--voxel 0.04] [--depth median|expected]
                                    [--keep-clusters K] [--min-faces M] [--normals] [--out mesh.ply]

A synthetic scene with LucidDreamer's statistics (synthetic.make_cloud "shell": one layer of pixel-sized Gaussians on a band
around the origin, made opaque here) is rendered from the rotate360 camera path; tsdf.fuse_views integrates every view's median
depth and colour into a volume around the band, eight views per launch, without a host copy; extract_mesh welds the zero crossing
into a mesh and save_mesh_ply writes it.  --keep-clusters K and --min-faces M clean the mesh on the device (mesh.filter_clusters:
the K largest connected components, none below M faces, degenerate faces dropped; 2DGS uses 50 and 50), --normals adds
mesh.vertex_normals to the file; without the three the mesh is written as extracted.  This is what the surface-reconstruction
code bases do with Open3D on the host after training with the depth, normal and distortion regularisers.  Needs a HIP device.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from luciddreamer_amd import cameras, mesh, synthetic, tsdf  # noqa: E402
from luciddreamer_amd.gaussian_renderer import DEFAULT_OPT, GaussianCloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=400_000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--views", type=int, default=30)
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--depth", choices=("median", "expected"), default="median")
    ap.add_argument("--keep-clusters", type=int, default=0, help="keep the K largest connected components (0: all)")
    ap.add_argument("--min-faces", type=int, default=1, help="drop components with fewer faces")
    ap.add_argument("--normals", action="store_true", help="write vertex normals")
    ap.add_argument("--out", default="mesh.ply")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("examples/extract_mesh.py needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    c = synthetic.make_cloud(a.points, "shell", seed=0, sh_coeffs=1)
    pc = GaussianCloud(c["means3D"].to(dev), c["scales"].to(dev), c["rotations"].to(dev), torch.full_like(c["opacities"], 0.99).to(dev),
                       c["shs"].to(dev), active_sh_degree=0, requires_grad=False)
    views = [v.to(dev) for v in cameras.rotate360_path(a.size, a.size, n_views=a.views)]
    # the band: radius 2.2 .. 3.9 in x and z, |y| below 1.4
    lo, hi = (-4.2, -1.6, -4.2), (4.2, 1.6, 4.2)
    dims = tuple(int(round((h - l) / a.voxel)) + 1 for l, h in zip(lo, hi))
    volume = tsdf.TSDFVolume(lo, a.voxel, dims, 4.0 * a.voxel, dev)
    bg = torch.zeros(3, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tsdf.fuse_views(volume, views, pc, DEFAULT_OPT, bg, depth=a.depth, alpha_min=0.5)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    vertices, colors, faces = volume.extract_mesh(min_weight=1.0)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    seen = int((volume.weight > 0).sum())
    print(f"{len(views)} views of {a.size} x {a.size} into {dims[0]} x {dims[1]} x {dims[2]} voxels: {seen} observed, "
          f"render + fuse {1e3 * (t1 - t0):.1f} ms, extract {1e3 * (t2 - t1):.1f} ms")
    if a.keep_clusters > 0 or a.min_faces > 1:
        n_before = faces.shape[0]
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        vertices, faces, colors = mesh.filter_clusters(vertices, faces, colors=colors, keep_largest=a.keep_clusters,
                                                       min_faces=a.min_faces, drop_degenerate=True)
        torch.cuda.synchronize()
        print(f"clean-up: {n_before - faces.shape[0]} of {n_before} faces removed, {1e3 * (time.perf_counter() - t3):.1f} ms")
    normals = mesh.vertex_normals(vertices, faces) if a.normals else None
    print(f"mesh: {vertices.shape[0]} vertices, {faces.shape[0]} faces{', normals' if a.normals else ''} -> {a.out}")
    tsdf.save_mesh_ply(a.out, vertices, colors, faces, normals=normals)


if __name__ == "__main__":
    main()
