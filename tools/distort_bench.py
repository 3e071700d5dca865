"""Cost of the depth distortion pass (lr_render_distortion) and of its backward (lr_distortion_backward) against the blend forward,
the depth-mode blend backward and the per-Gaussian backward of the same view.

    python tools/distort_bench.py [--iters 25] [--warmup 5] [--workloads c3,ld512] [--view 0] [--map ndc]

For each workload (bench.py's C3 and LD-512 clouds and cameras, one view of the rotate360 path) one exact-mode forward is run
through the binding; on its buffers the distortion pass and its whole backward are timed with HIP events around ten calls back to
back (per call; median of --iters after --warmup).  The library's per-stage events give, in the same process, the blend forward
(render_fwd), the depth-mode blend backward (render_bwd) and its per-Gaussian backward (gauss_bwd) over --iters forwards and
depth-mode backwards of the same view, and -- over --iters distortion backwards -- k_distort_bwd (recorded as that call's render_bwd
stage) and the per-Gaussian backward behind it.  Prints ONE JSON line; times in microseconds.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

INNER = 10
WORKLOADS = {"c3": ("band", 1_000_000, (1920, 1080)), "ld512": ("shell", 1_000_000, (512, 512))}


def _time_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):                  # back to back: the interval is the kernels', not one call's host time
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / INNER)
    return round(statistics.median(times), 1)


def _stages(fn, iters):
    from luciddreamer_amd import _lib
    _lib.profile_enable(True)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    st = _lib.profile_read()
    _lib.profile_enable(False)
    return lambda k: round(st[k][0] / max(1, st[k][1]) * 1000.0, 1) if k in st and st[k][1] else None


def run(name, view, iters, warmup, mapping, dev):
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
    gc = synthetic.upstream_grad(H, W).to(dev)
    gz = torch.randn(1, H, W, generator=torch.Generator().manual_seed(4)).to(dev)

    def depth_backward():
        return _C.rasterize_gaussians_backward(bg, c["means3D"], radii, None, c["scales"], c["rotations"], 1.0, None,
                                               cam.world_view_transform, cam.full_proj_transform, tfx, tfy, gc, gz, c["shs"], 3,
                                               cam.camera_center, geom, R, binning, img, False, skip_unused=True, depth_image=depth)

    def both():
        forward()
        depth_backward()
    per = _stages(both, iters)

    dist, mom = _C.render_distortion(geom, binning, img, P, H, W, distortion_map=mapping)
    gd = torch.randn(1, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    acc = dict(means2D=torch.zeros(P, 3, device=dev), opacity=torch.zeros(P, 1, device=dev), means3D=torch.zeros(P, 3, device=dev),
               scales=torch.zeros(P, 3, device=dev), rotations=torch.zeros(P, 4, device=dev))
    inputs = dict(means3D=c["means3D"], scales=c["scales"], rotations=c["rotations"])

    def dist_backward():
        _C.distortion_backward(geom, binning, img, gd, dist, mom, rs, distortion_map=mapping, accumulate_into=acc, **inputs)
    per_d = _stages(dist_backward, iters)
    res = dict(instances=int(R), pixels_with_distortion=round(float((dist > 0).float().mean()), 4),
               render_fwd_us=per("render_fwd"), depth_render_bwd_us=per("render_bwd"), depth_gauss_bwd_us=per("gauss_bwd"),
               distort_fwd_us=_time_us(lambda: _C.render_distortion(geom, binning, img, P, H, W, distortion_map=mapping), iters, warmup),
               k_distort_bwd_us=per_d("render_bwd"), distort_gauss_bwd_us=per_d("gauss_bwd"),
               distortion_backward_us=_time_us(dist_backward, iters, warmup),
               fwd_shape=_lib.last_launch_shapes()[0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default="c3,ld512")
    ap.add_argument("--view", type=int, default=0)
    ap.add_argument("--map", default="ndc", choices=("ndc", "linear"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib
    out = dict(tool="distort_bench", iters=args.iters, warmup=args.warmup, view=args.view, map=args.map,
               version=_lib.lib().lr_version().decode())
    for name in args.workloads.split(","):
        out[name] = run(name, args.view, args.iters, args.warmup, args.map, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
