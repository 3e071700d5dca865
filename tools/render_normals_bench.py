"""Cost of the rendered normal map pass (lr_render_normals) and of its backward (lr_render_normals_backward) against the blend
forward and the distortion pair of the same view.

    python tools/render_normals_bench.py [--iters 25] [--warmup 5] [--workloads c3,ld512] [--view 0]

For each workload (bench.py's C3 and LD-512 clouds and cameras, one view of the rotate360 path) one exact-mode forward is run
through the binding; on its buffers the normal pass (per-Gaussian normals + the walk) and its whole backward are timed with HIP
events around ten calls back to back (per call; median of --iters after --warmup), and so is the distortion pair, in the same
process.  The library's per-stage events give the blend forward (render_fwd) over --iters forwards, and -- over --iters normal
backwards -- k_normals_bwd (recorded as that call's render_bwd stage) and the per-Gaussian stage behind it (k_gauss_bwd and
k_normal_rot_bwd, recorded as gauss_bwd).  Prints ONE JSON line; times in microseconds.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.distort_bench import WORKLOADS, _stages, _time_us      # noqa: E402


def run(name, view, iters, warmup, dev):
    from types import SimpleNamespace
    from luciddreamer_amd import _C, _lib, cameras, synthetic
    kind, P, (W, H) = WORKLOADS[name]
    c = {k: v.to(dev).contiguous() for k, v in synthetic.make_cloud(P, kind, 0).items()}
    cam = cameras.rotate360_path(W, H, n_views=30)[view].to(dev)
    bg = torch.zeros(3, device=dev)
    tfx, tfy = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    rs = SimpleNamespace(image_height=H, image_width=W, tanfovx=tfx, tanfovy=tfy, scale_modifier=1.0,
                         viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center)

    def forward():
        return _C.rasterize_gaussians(bg, c["means3D"], None, c["opacities"], c["scales"], c["rotations"], 1.0, None,
                                      cam.world_view_transform, cam.full_proj_transform, tfx, tfy, H, W, c["shs"], 3,
                                      cam.camera_center, False, False)
    R, color, depth, radii, geom, binning, img = forward()
    per = _stages(forward, iters)
    inputs = dict(means3D=c["means3D"], scales=c["scales"], rotations=c["rotations"])
    acc = dict(means2D=torch.zeros(P, 3, device=dev), opacity=torch.zeros(P, 1, device=dev), means3D=torch.zeros(P, 3, device=dev),
               scales=torch.zeros(P, 3, device=dev), rotations=torch.zeros(P, 4, device=dev))

    normals, gauss_normals = _C.render_normals(geom, binning, img, radii, rs, **inputs)
    gn = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)

    def normals_backward():
        _C.render_normals_backward(geom, binning, img, gn, normals, gauss_normals, radii, rs, accumulate_into=acc, **inputs)
    per_n = _stages(normals_backward, iters)

    dist, mom = _C.render_distortion(geom, binning, img, P, H, W)
    gd = torch.randn(1, H, W, generator=torch.Generator().manual_seed(3)).to(dev)

    def dist_backward():
        _C.distortion_backward(geom, binning, img, gd, dist, mom, rs, accumulate_into=acc, **inputs)
    return dict(instances=int(R), pixels_with_a_normal=round(float((normals != 0).any(dim=0).float().mean()), 4),
                render_fwd_us=per("render_fwd"),
                normals_fwd_us=_time_us(lambda: _C.render_normals(geom, binning, img, radii, rs, **inputs), iters, warmup),
                k_normals_bwd_us=per_n("render_bwd"), normals_gauss_stage_us=per_n("gauss_bwd"),
                normals_backward_us=_time_us(normals_backward, iters, warmup),
                distort_fwd_us=_time_us(lambda: _C.render_distortion(geom, binning, img, P, H, W), iters, warmup),
                distortion_backward_us=_time_us(dist_backward, iters, warmup),
                fwd_shape=_lib.last_launch_shapes()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default="c3,ld512")
    ap.add_argument("--view", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib
    out = dict(tool="render_normals_bench", iters=args.iters, warmup=args.warmup, view=args.view,
               version=_lib.lib().lr_version().decode())
    for name in args.workloads.split(","):
        out[name] = run(name, args.view, args.iters, args.warmup, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
