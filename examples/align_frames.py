"""The point-cloud stage of LucidDreamer.generate_pcd (R/luciddreamer.py:363-570) on the device, on synthetic data.

    python examples/align_frames.py [--size 256] [--poses 4] [--depth-scale 1.1]

One synthetic RGB-D view (luciddreamer_amd.synthetic.rgbd_view) is lifted into a cloud.  For every dream pose the accumulated
cloud is projected into the new view (reproject.project: warped image + hole mask).  Where the reference would now run its
inpainting and depth networks, this example takes the synthetic view's own colours, and its depth with a wrong scale and a
smooth offset (synthetic.miscalibrated_depth: what a monocular depth network hands back).  reproject.dream_step then does what
follows the networks (R/luciddreamer.py:424-493) on the device: it fits the scale, measures the depth offsets along the hole's
border, interpolates them into the holes, lifts the corrected depth and appends the hole pixels.  Then reproject.align_frames
renders the training frames: every dream pose seen from 5 inner poses.  Needs a HIP device; no network, no scipy.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from luciddreamer_amd import reproject, synthetic  # noqa: E402


def yaw_pose(angle, shift):
    """World to camera: a turn about the y axis and a sideways step."""
    c, s = math.cos(angle), math.sin(angle)
    P = np.eye(4)
    P[:3, :3] = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    P[0, 3] = shift
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--poses", type=int, default=4)
    ap.add_argument("--depth-scale", type=float, default=1.1, help="the stand-in depth network is off by this factor")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("examples/align_frames.py needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    H = W = a.size
    fov_x = math.radians(60.0)
    focal = 0.5 * W / math.tan(0.5 * fov_x)
    K = np.array([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1]])
    image, depth = (t.to(dev) for t in synthetic.rgbd_view(H, W))
    render_poses = np.stack([yaw_pose(0.06 * i, -0.15 * i) for i in range(a.poses)])
    inner_poses = np.stack([yaw_pose(0.0, 0.0)] + [yaw_pose(0.03 * s, 0.05 * t) for s, t in ((1, 1), (1, -1), (-1, 1), (-1, -1))])

    points = reproject.lift(depth, K, render_poses[0, :3, :3], render_poses[0, :3, 3:4])          # [3, H*W]
    colors = image.reshape(-1, 3).contiguous()
    print(f"view 0: {points.shape[1]} points lifted from a {H} x {W} RGB-D view")
    net_depth = synthetic.miscalibrated_depth(depth, scale=a.depth_scale)                          # the depth "network"
    border_error = lambda comp: float(comp.corr_value[:comp.n_corr].abs().nanmean()) if comp.n_corr else 0.0
    for i in range(1, a.poses):
        R, T = render_poses[i, :3, :3], render_poses[i, :3, 3:4]
        f = reproject.project(points, colors, K, R, T, H, W)
        hole = f.mask == 0
        # cloud-to-depth distance along the camera rays of the border points, before (scale 1) and after the fit
        before = border_error(reproject.compensate(points, f, net_depth, K, R, T, scale=1.0))
        old = points
        points, colors, info = reproject.dream_step(points, colors, f, image, net_depth, K, R, T)
        after = border_error(reproject.compensate(old, f, net_depth, K, R, T, scale=info.scale))
        print(f"dream pose {i}: {int(f.valid.sum())} of {f.valid.numel()} points on screen, {int(f.mask.sum())} mask pixels, "
              f"{int(hole.sum())} hole pixels ({100.0 * float(hole.float().mean()):.1f} %), {int(f.border.sum())} border pixels, "
              f"cloud now {points.shape[1]} points")
        print(f"    fitted scale {info.scale:.4f} over {info.fit.n_used} points (mse {info.fit.mse_before:.4g} -> "
              f"{info.fit.mse_after:.4g}); {info.n_corr} border correspondences, mean |cloud - depth| along the border "
              f"{before:.4f} -> {after:.4f}; {info.n_added} points appended")

    data = reproject.align_frames(points, colors, K, render_poses, inner_poses, H, W, fov_x, as_tensors=True)
    frames = torch.stack([f["image"] for f in data["frames"]])
    empty = (frames == 0).all(dim=-1).float().mean(dim=(1, 2))
    print(f"align_frames: {len(data['frames'])} frames of {data['H']} x {data['W']} from {data['pcd_points'].shape[1]} points; "
          f"empty pixels per frame min {100 * float(empty.min()):.1f} % / mean {100 * float(empty.mean()):.1f} % / "
          f"max {100 * float(empty.max()):.1f} %")


if __name__ == "__main__":
    main()
