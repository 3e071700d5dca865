"""Cost of anti-aliasing (config.set_antialiasing -> lr_set_antialiasing), off against on.

    python tools/aa_bench.py [--iters 25] [--warmup 5] [--steps 10] [--workloads c3,ld512] [--streams 3]

For each workload (bench.py's C3 and LD-512 clouds and cameras):
  one view    a forward + backward through the compiled node, timed with HIP events (median of --iters after --warmup), then the
              same loop under the library's per-stage events: preprocess, blend forward, blend backward, per-Gaussian backward;
              the view's header counts: num_rendered (the reference's rectangle count, which the setting does not move) and
              num_instances (tile instances after exact tile culling, which the smaller opacities shorten);
  30 views    the ViewBatch step (lr_views_accumulate), views per second.
Prints ONE JSON line.
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


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def run(name, args, dev):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd import _C, _lib, cameras, config, parallel, synthetic
    kind, P, (W, H) = WORKLOADS[name]
    c = {k: v.to(dev).contiguous() for k, v in synthetic.make_cloud(P, kind, 0).items()}
    cams = [cam.to(dev) for cam in cameras.rotate360_path(W, H, n_views=30)]
    cam = cams[3]
    bg = torch.zeros(3, device=dev)
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0,
                                       cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center, False, False)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    gc = synthetic.upstream_grad(H, W).to(dev)
    res = {}
    for on in (False, True):
        config.set_antialiasing(on)
        try:
            # header counts of the view, exact mode
            config.set_async(False)
            with torch.no_grad():
                fwd = _C.rasterize_gaussians(bg, c["means3D"], None, c["opacities"], c["scales"], c["rotations"], 1.0, None,
                                             cam.world_view_transform, cam.full_proj_transform, rs.tanfovx, rs.tanfovy, H, W,
                                             c["shs"], 3, cam.camera_center, False, False)
            hdr = fwd[4][:64].cpu().view(torch.int32)
            config.set_async(True)
            config.reset()
            config.set_antialiasing(on)

            def step():
                m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
                col = GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"],
                                             shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rotations"])[0]
                torch.autograd.grad([col], [m2] + list(leaves.values()), [gc])
            ms = _time(step, args.iters, args.warmup)
            _lib.profile_enable(True)
            for _ in range(args.iters):
                step()
            torch.cuda.synchronize()
            st = _lib.profile_read()
            _lib.profile_enable(False)
            per = lambda k: round(st[k][0] / max(1, st[k][1]) * 1000.0, 1) if k in st and st[k][1] else None
            one = dict(fwd_bwd_ms=round(ms, 4), preprocess_us=per("preprocess"), render_fwd_us=per("render_fwd"),
                       render_bwd_us=per("render_bwd"), gauss_bwd_us=per("gauss_bwd"), num_rendered=int(hdr[0]),
                       num_instances=int(hdr[6]))
            # the 30-view step
            cap = int(int(hdr[6]) * 2.0) + 65536
            acc = {"means3D": torch.zeros(P, 3, device=dev), "means2D": torch.zeros(P, 3, device=dev),
                   "opacity": torch.zeros(P, 1, device=dev), "sh": torch.zeros_like(c["shs"]),
                   "scales": torch.zeros(P, 3, device=dev), "rotations": torch.zeros(P, 4, device=dev)}
            batch = parallel.ViewBatch(cams, [gc] * len(cams), 3, bg, cap, n_streams=args.streams)

            def views():
                batch.run(c["means3D"], c["opacities"], c["scales"], c["rotations"], c["shs"], acc)
            vms = _time(views, args.steps, max(2, args.warmup // 2))
            batch.check()
            batch.release_workspace()
            res["on" if on else "off"] = dict(one_view=one, views30=dict(step_ms=round(vms, 3),
                                                                        views_per_s=round(len(cams) / vms * 1e3, 1)))
        finally:
            config.set_async(True)
            config.reset()
    res["on_over_off"] = dict(
        fwd_bwd=round(res["on"]["one_view"]["fwd_bwd_ms"] / res["off"]["one_view"]["fwd_bwd_ms"], 3),
        views30=round(res["on"]["views30"]["step_ms"] / res["off"]["views30"]["step_ms"], 3),
        num_instances=round(res["on"]["one_view"]["num_instances"] / max(1, res["off"]["one_view"]["num_instances"]), 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--workloads", default="c3,ld512")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib
    out = dict(tool="aa_bench", iters=args.iters, warmup=args.warmup, version=_lib.lib().lr_version().decode())
    for name in args.workloads.split(","):
        out[name] = run(name, args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
