"""Cost of depth supervision in the multi-view step (parallel.ViewBatch), and of the masked depth L1 kernels alone.

    python tools/views_depth_bench.py [--steps 10] [--warmup 3] [--views 30] [--streams 3] [--workloads c3,ld512]

For each workload (bench.py's C3 and LD-512 clouds, --views views of the rotate360 path, ONE ViewBatch call per step over
--streams chains, async mode with the capacity bench.py would give) four steps are timed with HIP events (median of --steps after
--warmup): `default` (lr_views_accumulate with grad_colors) against `depth` (with grad_colors + grad_depths),
and `train` (with targets) against `train_depth` (with targets + depth_targets).
Then lr_depth_l1_forward + lr_depth_l1_backward alone at 1080p and 512x512 (median of 200 timed pairs).  Prints ONE JSON line.
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

WORKLOADS = {"c3": ("band", 1_000_000, (1920, 1080)), "ld512": ("shell", 1_000_000, (512, 512))}


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def capacity(c, cams, bg, W, H):
    """The async-mode capacity bench.py uses: 1.25 x the largest exact-mode instance count of the path, + 4096."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd import _C, config
    config.set_async(False)
    n = []
    with torch.no_grad():
        for cam in cams:
            rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0,
                                               cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center,
                                               False, False)
            GaussianRasterizer(rs)(means3D=c["means3D"], means2D=torch.zeros_like(c["means3D"]), opacities=c["opacities"],
                                   shs=c["shs"], scales=c["scales"], rotations=c["rotations"])
            n.append(int(_C.last_num_rendered()))
    config.set_async(True)
    config.reset()
    return int(max(n) * 1.25) + 4096


def run(name, args, dev):
    from luciddreamer_amd import cameras, parallel, synthetic
    kind, P, (W, H) = WORKLOADS[name]
    c = {k: v.to(dev).contiguous() for k, v in synthetic.make_cloud(P, kind, 0).items()}
    cams = [cc.to(dev) for cc in cameras.rotate360_path(W, H, n_views=args.views)]
    bg = torch.zeros(3, device=dev)
    cap = capacity(c, cams, bg, W, H)
    gc = synthetic.upstream_grad(H, W).to(dev)
    gen = torch.Generator().manual_seed(3)
    gds = [torch.randn(1, H, W, generator=gen).to(dev) for _ in cams]
    targets = [torch.rand(3, H, W, generator=gen).to(dev) for _ in cams]
    dts = [(2.0 + 6.0 * torch.rand(1, H, W, generator=gen)).to(dev) for _ in cams]
    acc = {"means3D": torch.zeros(P, 3, device=dev), "means2D": torch.zeros(P, 3, device=dev),
           "opacity": torch.zeros(P, 1, device=dev), "sh": torch.zeros_like(c["shs"]), "scales": torch.zeros(P, 3, device=dev),
           "rotations": torch.zeros(P, 4, device=dev)}
    V, S = len(cams), args.streams
    batches = {
        "default": parallel.ViewBatch(cams, [gc] * V, 3, bg, cap, n_streams=S),
        "depth": parallel.ViewBatch(cams, [gc] * V, 3, bg, cap, n_streams=S, grad_depths=gds),
        "train": parallel.ViewBatch(cams, None, 3, bg, cap, n_streams=S, targets=targets),
        "train_depth": parallel.ViewBatch(cams, None, 3, bg, cap, n_streams=S, targets=targets, depth_targets=dts,
                                          depth_weight=0.5),
    }
    res = {"views": V, "streams": S, "capacity": cap}
    for mode, b in batches.items():
        def step():
            b.run(c["means3D"], c["opacities"], c["scales"], c["rotations"], c["shs"], acc)
        ms = _time(step, args.steps, args.warmup)
        b.check()
        res[mode] = {"step_ms": round(ms, 3), "views_per_s": round(V / ms * 1e3, 1)}
        b.release_workspace()                           # one workspace at a time
    res["depth_over_default"] = round(res["depth"]["step_ms"] / res["default"]["step_ms"], 3)
    res["train_depth_over_train"] = round(res["train_depth"]["step_ms"] / res["train"]["step_ms"], 3)
    return res


def depth_l1_kernel(H, W, dev):
    from luciddreamer_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(5)
    d = (1.0 + torch.rand(H, W, generator=gen)).to(dev)
    t = (1.0 + torch.rand(H, W, generator=gen)).to(dev)
    out = torch.empty(1, device=dev)
    grad = torch.empty_like(d)
    ws = torch.empty(int(L.lr_depth_l1_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def fwd():
        L.lr_depth_l1_forward(H, W, d.data_ptr(), t.data_ptr(), 1.0, out.data_ptr(), ws.data_ptr(), ws.numel(), s)

    def bwd():
        L.lr_depth_l1_backward(H, W, d.data_ptr(), t.data_ptr(), 1.0, None, grad.data_ptr(), s)
    f = _time(fwd, 200, 20)
    b = _time(bwd, 200, 20)
    return {"forward_us": round(f * 1e3, 1), "backward_us": round(b * 1e3, 1), "fwd_plus_bwd_us": round((f + b) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=30)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--workloads", default="c3,ld512")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib
    out = {"tool": "views_depth_bench", "steps": args.steps, "warmup": args.warmup,
           "version": _lib.lib().lr_version().decode()}
    for name in args.workloads.split(","):
        out[name] = run(name, args, dev)
        torch.cuda.empty_cache()
    out["depth_l1"] = {"1080p": depth_l1_kernel(1080, 1920, dev), "512": depth_l1_kernel(512, 512, dev)}
    print(json.dumps(out, separators=(",", ":")))


if __name__ == "__main__":
    main()
