"""Cost of the densification statistics in the multi-view step (parallel.ViewBatch(densify_stats=...)).

    python tools/views_stats_bench.py [--rounds 8] [--warmup 3] [--views 30] [--streams 3]

One process, the C3 step (bench.py's 1 M "band" cloud, 1080p, --views views of the rotate360 path, ONE ViewBatch call per step
over --streams chains, async mode with the capacity bench.py would give), three variants: `none` (lr_views_accumulate without
the stat_* members), `grad` and `absgrad`.  The variants are ALTERNATED: every round times one step of each, in an order that
rotates from round to round, so that clock and thermal drift fall on all three alike; --warmup rounds are run and discarded
first.  HIP-event times; per variant the median step, the spread (min, max) and views/s.  The gradient accumulators and the three
statistics tensors are zeroed outside the timed region.  Prints ONE JSON line.
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

KIND, P, (W, H) = "band", 1_000_000, (1920, 1080)
VARIANTS = ("none", "grad", "absgrad")


def capacity(c, cams, bg):
    """The async-mode capacity bench.py uses: 1.25 x the largest exact-mode instance count of the path, + 4096."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd import _C, config
    config.set_async(False)
    n = []
    try:
        with torch.no_grad():
            for cam in cams:
                rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0,
                                                   cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center,
                                                   False, False)
                GaussianRasterizer(rs)(means3D=c["means3D"], means2D=torch.zeros_like(c["means3D"]), opacities=c["opacities"],
                                       shs=c["shs"], scales=c["scales"], rotations=c["rotations"])
                n.append(int(_C.last_num_rendered()))
    finally:
        config.set_async(True)
        config.reset()
    return int(max(n) * 1.25) + 4096


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=30)
    ap.add_argument("--streams", type=int, default=3)
    args = ap.parse_args()
    from luciddreamer_amd import _lib, cameras, parallel, synthetic
    dev = torch.device("cuda:0")
    c = {k: v.to(dev).contiguous() for k, v in synthetic.make_cloud(P, KIND, 0).items()}
    cams = [cc.to(dev) for cc in cameras.rotate360_path(W, H, n_views=args.views)]
    bg = torch.zeros(3, device=dev)
    cap = capacity(c, cams, bg)
    g = synthetic.upstream_grad(H, W).to(dev)
    acc = {"means3D": torch.zeros(P, 3, device=dev), "means2D": torch.zeros(P, 3, device=dev),
           "opacity": torch.zeros(P, 1, device=dev), "sh": torch.zeros_like(c["shs"]), "scales": torch.zeros(P, 3, device=dev),
           "rotations": torch.zeros(P, 4, device=dev)}
    stats = {"xyz_gradient_accum": torch.zeros(P, 1, device=dev), "denom": torch.zeros(P, 1, device=dev),
             "max_radii2D": torch.zeros(P, device=dev)}
    V = len(cams)
    # one workspace for the three: the statistics need no bytes of their own
    batches = {v: parallel.ViewBatch(cams, [g] * V, 3, bg, cap, n_streams=args.streams, densify_stats=None if v == "none" else v)
               for v in VARIANTS}
    ws = torch.empty(batches["none"].workspace_bytes(P), dtype=torch.uint8, device=dev)
    for b in batches.values():
        b.use_workspace(ws, P)

    def step(v):
        for t in (*acc.values(), *stats.values()):
            t.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        batches[v].run(c["means3D"], c["opacities"], c["scales"], c["rotations"], c["shs"], acc, stats=None if v == "none" else stats)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {v: [] for v in VARIANTS}
    for r in range(args.warmup + args.rounds):
        for k in range(len(VARIANTS)):
            v = VARIANTS[(r + k) % len(VARIANTS)]
            ms = step(v)
            if r >= args.warmup:
                times[v].append(ms)
    for b in batches.values():
        b.check()
    out = {"tool": "views_stats_bench", "rounds": args.rounds, "warmup": args.warmup, "views": V, "streams": args.streams,
           "capacity": cap, "version": _lib.lib().lr_version().decode()}
    for v in VARIANTS:
        med = statistics.median(times[v])
        out[v] = {"step_ms": round(med, 3), "min_ms": round(min(times[v]), 3), "max_ms": round(max(times[v]), 3),
                  "views_per_s": round(V / med * 1e3, 1)}
    for v in VARIANTS[1:]:
        out[v + "_over_none"] = round(out[v]["step_ms"] / out["none"]["step_ms"], 4)
    print(json.dumps(out, separators=(",", ":")))


if __name__ == "__main__":
    main()
