"""Cost of the median depth pass (lr_render_median) and of its gather backward (lr_median_backward) against the blend forward
and the per-Gaussian backward of the same view.

    python tools/median_bench.py [--iters 25] [--warmup 5] [--workloads c3,ld512] [--view 0]

For each workload (bench.py's C3 and LD-512 clouds and cameras, one view of the rotate360 path) one exact-mode forward is run
through the binding; on its buffers the median pass and its backward are timed with HIP events around ten calls back to back
(per call; median of --iters after --warmup).  The library's per-stage events over --iters forwards and backwards of the same view give the blend
forward (render_fwd) and the per-Gaussian backward (gauss_bwd) alone.  Prints ONE JSON line; times in microseconds.
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


def run(name, view, iters, warmup, dev):
    from luciddreamer_amd import _C, _lib, cameras, synthetic
    kind, P, (W, H) = WORKLOADS[name]
    c = {k: v.to(dev).contiguous() for k, v in synthetic.make_cloud(P, kind, 0).items()}
    cam = cameras.rotate360_path(W, H, n_views=30)[view].to(dev)
    bg = torch.zeros(3, device=dev)
    tfx, tfy = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)

    def forward():
        return _C.rasterize_gaussians(bg, c["means3D"], None, c["opacities"], c["scales"], c["rotations"], 1.0, None,
                                      cam.world_view_transform, cam.full_proj_transform, tfx, tfy, H, W, c["shs"], 3,
                                      cam.camera_center, False, False)
    R, color, depth, radii, geom, binning, img = forward()
    gc = synthetic.upstream_grad(H, W).to(dev)

    def backward():
        return _C.rasterize_gaussians_backward(bg, c["means3D"], radii, None, c["scales"], c["rotations"], 1.0, None,
                                               cam.world_view_transform, cam.full_proj_transform, tfx, tfy, gc, None, c["shs"], 3,
                                               cam.camera_center, geom, R, binning, img, False, skip_unused=True)
    _lib.profile_enable(True)
    for _ in range(iters):
        forward()
        backward()
    torch.cuda.synchronize()
    st = _lib.profile_read()
    _lib.profile_enable(False)
    per = lambda k: round(st[k][0] / max(1, st[k][1]) * 1000.0, 1) if k in st and st[k][1] else None

    md, ids = _C.render_median(geom, binning, img, P, H, W)
    gm = torch.randn(1, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    grad = torch.zeros(P, 3, device=dev)
    res = dict(instances=int(R), median_defined=round(float((ids >= 0).float().mean()), 4),
               render_fwd_us=per("render_fwd"), render_bwd_us=per("render_bwd"), gauss_bwd_us=per("gauss_bwd"),
               median_fwd_us=_time_us(lambda: _C.render_median(geom, binning, img, P, H, W), iters, warmup),
               median_bwd_us=_time_us(lambda: _C.median_backward(geom, binning, img, radii, ids, gm, cam.world_view_transform,
                                                                 accumulate_into=grad), iters, warmup),
               fwd_shape=_lib.last_launch_shapes()[0])
    return res


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
    out = dict(tool="median_bench", iters=args.iters, warmup=args.warmup, view=args.view, version=_lib.lib().lr_version().decode())
    for name in args.workloads.split(","):
        out[name] = run(name, args.view, args.iters, args.warmup, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
