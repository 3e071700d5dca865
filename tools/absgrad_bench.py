"""Cost of the absgrad-mode backward (config.set_absgrad -> lr_view_backward with dL_dmean2D_abs) against the default and the depth-mode backward.

    python tools/absgrad_bench.py [--iters 25] [--warmup 5] [--workloads c3,ld512]

tools/depth_grad_bench.py with two more modes: for each workload (bench.py's C3 and LD-512 clouds and cameras, one view) ONE
forward per mode is run through the compiled node and its backward is timed again and again on the retained graph (HIP events
around each backward, median of --iters after --warmup) -- default, depth (colour + depth loss), absgrad (colour loss) and
absgrad + depth.  A second pass with the library's per-stage events gives the blend backward (render_bwd) and the per-Gaussian
backward (gauss_bwd) alone; under `rocprofv3 --kernel-trace --stats` the same run gives the per-kernel times.  Prints ONE JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = {"c3": ("band", 1_000_000, (1920, 1080)), "ld512": ("shell", 1_000_000, (512, 512))}


def run(name, iters, warmup, dev):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd import _lib, cameras, config, synthetic
    kind, P, (W, H) = WORKLOADS[name]
    c = synthetic.make_cloud(P, kind, 0)
    cam = cameras.rotate360_path(W, H, n_views=30)[3].to(dev)
    import math
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, device=dev), 1.0,
                                       cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center, False, False)
    leaves = {k: c[k].to(dev).contiguous().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    gc = synthetic.upstream_grad(H, W).to(dev)
    gd = torch.randn(1, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    res = {}
    for mode in ("default", "depth", "absgrad", "absgrad_depth"):
        config.set_depth_gradient(mode.endswith("depth"))
        config.set_absgrad(mode.startswith("absgrad"))
        try:
            m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
            color, _, depth = GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"],
                                                     shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rotations"])
        finally:
            config.set_depth_gradient(False)
            config.set_absgrad(False)
        outs, grads = ([color, depth], [gc, gd]) if mode.endswith("depth") else ([color], [gc])
        inputs = [m2] + list(leaves.values())

        def backward():
            torch.autograd.grad(outs, inputs, grads, retain_graph=True)
        for _ in range(warmup):
            backward()
        torch.cuda.synchronize()
        times = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            backward()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        _lib.profile_enable(True)
        for _ in range(iters):
            backward()
        torch.cuda.synchronize()
        st = _lib.profile_read()
        _lib.profile_enable(False)
        per = lambda k: round(st[k][0] / max(1, st[k][1]) * 1000.0, 1) if k in st and st[k][1] else None
        res[mode] = dict(backward_ms=round(statistics.median(times), 4), render_bwd_us=per("render_bwd"), gauss_bwd_us=per("gauss_bwd"))
    ratio = lambda x, d: dict(
        backward=round(x["backward_ms"] / d["backward_ms"], 3),
        render_bwd=round(x["render_bwd_us"] / d["render_bwd_us"], 3) if d["render_bwd_us"] and x["render_bwd_us"] else None)
    res["depth_over_default"] = ratio(res["depth"], res["default"])
    res["absgrad_over_default"] = ratio(res["absgrad"], res["default"])
    res["absgrad_over_depth"] = ratio(res["absgrad"], res["depth"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default="c3,ld512")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib
    out = dict(tool="absgrad_bench", iters=args.iters, warmup=args.warmup, version=_lib.lib().lr_version().decode())
    for name in args.workloads.split(","):
        out[name] = run(name, args.iters, args.warmup, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
