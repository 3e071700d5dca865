#!/usr/bin/env python
"""The video renderer's loop (R/luciddreamer.py:250-265) over a 201-view rotate360 path, C3 (1e6 Gaussians, 1920x1080) and
LD-512 (1e6, 512x512), printed as one JSON line:

  reference_loop : render() per view, then the reference's host post-processing: .cpu(), the numpy frame packing and the
                   numpy restatement of colorize (tests/video_ref.py, with the product's jet LUT: no matplotlib needed)
  device_loop    : luciddreamer_amd.video.iter_video_frames end to end, to host numpy arrays
  render_only    : render() per view and nothing else (the floor of both loops)
  kernels        : us per frame of each new kernel, from device events: frames_to_uint8, colorize_depth with the on-device
                   percentile select, colorize_depth with fixed limits (the colouring pass alone); one frame and a batch of 8

    python tools/video_bench.py [--views 201] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from luciddreamer_amd import _lib, cameras, synthetic                  # noqa: E402
from luciddreamer_amd.gaussian_renderer import GaussianCloud, render  # noqa: E402
from luciddreamer_amd.video import colorize_depth, frames_to_uint8, iter_video_frames, jet_lut  # noqa: E402
from tests import video_ref as vr                                     # noqa: E402

CFGS = {"c3": ("band", 1_000_000, (1920, 1080)), "ld512": ("shell", 1_000_000, (512, 512))}


def event_us(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def run(cfg, n_views, reps, dev):
    kind, P, (W, H) = CFGS[cfg]
    c = synthetic.make_cloud(P, kind, 0)
    pc = GaussianCloud(c["means3D"].to(dev), c["scales"].to(dev), c["rotations"].to(dev), c["opacities"].to(dev),
                       c["shs"].to(dev), requires_grad=False)
    views = [v.to(dev) for v in cameras.rotate360_path(W, H, n_views=n_views)]
    bg = torch.zeros(3, device=dev)
    lut = jet_lut()
    res = {"views": n_views, "resolution": f"{W}x{H}"}

    def render_only():
        for v in views:
            render(v, pc, None, bg, render_only=True)
    render_only()
    torch.cuda.synchronize()
    t = time.perf_counter()
    render_only()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    res["render_only"] = {"frames_per_s": round(n_views / dt, 1), "ms_per_frame": round(dt / n_views * 1e3, 3)}

    def reference_loop(vs):
        frames, depths = [], []
        for v in vs:
            out = render(v, pc, None, bg)
            frame, depth = out["render"], out["depth"]
            frames.append(np.round(frame.permute(1, 2, 0).detach().cpu().numpy().clip(0, 1) * 255.).astype(np.uint8))
            depths.append(-(depth * (depth > 0)).detach().cpu().numpy())
        return frames, [vr.colorize(d.squeeze(0), lut)[0] for d in depths]
    reference_loop(views[:2])
    t = time.perf_counter()
    ref_frames, ref_depths = reference_loop(views)
    dt = time.perf_counter() - t
    res["reference_loop"] = {"frames_per_s": round(n_views / dt, 2), "ms_per_frame": round(dt / n_views * 1e3, 3)}

    list(iter_video_frames(views[:4], pc, None, bg))
    torch.cuda.synchronize()
    t = time.perf_counter()
    got = list(iter_video_frames(views, pc, None, bg, in_flight=8))
    dt = time.perf_counter() - t
    res["device_loop"] = {"frames_per_s": round(n_views / dt, 1), "ms_per_frame": round(dt / n_views * 1e3, 3), "in_flight": 8}
    res["device_over_reference"] = round(res["device_loop"]["frames_per_s"] / res["reference_loop"]["frames_per_s"], 1)
    res["bytes_equal_to_reference_loop"] = all(np.array_equal(f, rf) and np.array_equal(d, rd)
                                               for (f, d), rf, rd in zip(got, ref_frames, ref_depths))

    with torch.no_grad():
        outs = [render(v, pc, None, bg, render_only=True) for v in views[:8]]
    img8 = torch.stack([o["render"] for o in outs]).contiguous()
    dep8 = torch.stack([o["depth"] for o in outs]).contiguous()
    fixed = (torch.tensor(-8.0, device=dev), torch.tensor(-1.0, device=dev))
    k = {}
    for label, img, dep, n in (("1", img8[0], dep8[0], 1), ("batch8", img8, dep8, 8)):
        k["frames_to_uint8_" + label] = round(event_us(lambda: frames_to_uint8(img), reps) / n, 1)
        k["colorize_select_" + label] = round(event_us(lambda: colorize_depth(dep), reps) / n, 1)
        k["colorize_fixed_" + label] = round(event_us(lambda: colorize_depth(dep, vmin=fixed[0], vmax=fixed[1]), reps) / n, 1)
    res["kernels_us_per_frame"] = k
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=201)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--configs", default="c3,ld512")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"tool": "video_bench", "version": _lib.lib().lr_version().decode()}
    for cfg in args.configs.split(","):
        out[cfg] = run(cfg, args.views, args.reps, dev)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
