"""Cost of the Pearson depth loss against the masked depth L1: the kernels alone, and inside the multi-view training step.

    python tools/depth_pearson_bench.py [--steps 10] [--warmup 3] [--views 30] [--streams 3] [--rounds 3] [--workloads c3,ld512]

Kernels: lr_depth_pearson_forward (two launches) + lr_depth_pearson_backward against lr_depth_l1_forward + lr_depth_l1_backward at
1080p and 512x512, each call timed with HIP events (median of 200 after 20), the two losses alternating.
Step: for each workload of tools/views_depth_bench.py (bench.py's C3 and LD-512 clouds, --views views, ONE ViewBatch call per step
with targets + depth_targets over --streams chains) depth_loss="l1" against depth_loss="pearson" on the same box, alternating
for --rounds rounds; the median over the rounds of the per-round medians is reported.  Prints ONE JSON line.
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

from tools.views_depth_bench import WORKLOADS, _time  # noqa: E402


def kernels(H, W, dev):
    from luciddreamer_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(5)
    d = (1.0 + torch.rand(H, W, generator=gen)).to(dev)
    t = (1.0 + torch.rand(H, W, generator=gen)).to(dev)
    out = torch.empty(2, device=dev)
    grad = torch.empty_like(d)
    ws = torch.empty(int(L.lr_depth_pearson_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    p = (H, W, d.data_ptr(), t.data_ptr(), 1.0)
    calls = {
        "l1_forward": lambda: L.lr_depth_l1_forward(*p, out.data_ptr(), ws.data_ptr(), ws.numel(), s),
        "pearson_forward": lambda: L.lr_depth_pearson_forward(*p, out.data_ptr(), ws.data_ptr(), ws.numel(), s),
        "l1_backward": lambda: L.lr_depth_l1_backward(*p, None, grad.data_ptr(), s),
        "pearson_backward": lambda: L.lr_depth_pearson_backward(*p, None, ws.data_ptr(), ws.numel(), grad.data_ptr(), s),
    }
    res = {}
    for name, fn in calls.items():                       # l1, pearson, l1, pearson; the Pearson backward finds its forward's record
        assert fn() == 0
        res[name + "_us"] = round(_time(fn, 200, 20) * 1e3, 1)
    res["l1_pair_us"] = round(res["l1_forward_us"] + res["l1_backward_us"], 1)
    res["pearson_trio_us"] = round(res["pearson_forward_us"] + res["pearson_backward_us"], 1)
    return res


def step(name, args, dev):
    from luciddreamer_amd import cameras, parallel, synthetic
    from tools.views_depth_bench import capacity
    kind, P, (W, H) = WORKLOADS[name]
    c = {k: v.to(dev).contiguous() for k, v in synthetic.make_cloud(P, kind, 0).items()}
    cams = [cc.to(dev) for cc in cameras.rotate360_path(W, H, n_views=args.views)]
    bg = torch.zeros(3, device=dev)
    cap = capacity(c, cams, bg, W, H)
    gen = torch.Generator().manual_seed(3)
    targets = [torch.rand(3, H, W, generator=gen).to(dev) for _ in cams]
    dts = [(2.0 + 6.0 * torch.rand(1, H, W, generator=gen)).to(dev) for _ in cams]
    acc = {"means3D": torch.zeros(P, 3, device=dev), "means2D": torch.zeros(P, 3, device=dev),
           "opacity": torch.zeros(P, 1, device=dev), "sh": torch.zeros_like(c["shs"]), "scales": torch.zeros(P, 3, device=dev),
           "rotations": torch.zeros(P, 4, device=dev)}
    V = len(cams)
    ms = {"l1": [], "pearson": []}
    for _ in range(args.rounds):
        for mode in ("l1", "pearson"):
            b = parallel.ViewBatch(cams, None, 3, bg, cap, n_streams=args.streams, targets=targets, depth_targets=dts,
                                   depth_weight=0.5, depth_loss=mode)
            ms[mode].append(_time(lambda: b.run(c["means3D"], c["opacities"], c["scales"], c["rotations"], c["shs"], acc),
                                  args.steps, args.warmup))
            b.check()
            b.release_workspace()                       # one workspace at a time
    res = {"views": V, "streams": args.streams, "capacity": cap, "rounds": args.rounds}
    for mode, v in ms.items():
        m = statistics.median(v)
        res[mode] = {"step_ms": round(m, 3), "views_per_s": round(V / m * 1e3, 1), "rounds_ms": [round(x, 3) for x in v]}
    res["pearson_over_l1"] = round(res["pearson"]["step_ms"] / res["l1"]["step_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=30)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default="c3,ld512")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib
    out = {"tool": "depth_pearson_bench", "steps": args.steps, "warmup": args.warmup, "version": _lib.lib().lr_version().decode(),
           "kernels": {"1080p": kernels(1080, 1920, dev), "512": kernels(512, 512, dev)}}
    for name in [w for w in args.workloads.split(",") if w]:
        out[name] = step(name, args, dev)
        torch.cuda.empty_cache()
    print(json.dumps(out, separators=(",", ":")))


if __name__ == "__main__":
    main()
