"""Cost of the alpha output (return_alpha -> lr_render_alpha, lr_view_backward with dL_dalpha) against the default backward and against the
two-render workaround.

    python tools/alpha_grad_bench.py [--iters 25] [--warmup 5] [--workloads c3,ld512]

For each workload (bench.py's C3 and LD-512 clouds and cameras, one view) ONE forward per mode is run through the compiled node
and its backward is then timed again and again on the retained graph (HIP events around each backward, median of --iters after
--warmup): default mode with a colour loss, alpha mode with a colour + alpha loss, and depth + alpha mode
(config.set_depth_gradient) with a colour + depth + alpha loss.  A second pass of the same loop with the library's per-stage
events gives the blend backward (render_bwd) and the per-Gaussian backward (gauss_bwd) alone.  Then:
  alpha_kernel_us     the forward's alpha pass alone (lr_render_alpha on the forward's image state), median over --iters;
  two_render          what the workaround adds per view: a whole second forward + backward (colors_precomp = ones,
                      background 0, channel 0 as alpha), against what alpha mode adds (the alpha pass + the backward's
                      difference to default mode).
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


def run(name, iters, warmup, dev):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd import _C, _lib, cameras, config, synthetic
    kind, P, (W, H) = WORKLOADS[name]
    c = synthetic.make_cloud(P, kind, 0)
    cam = cameras.rotate360_path(W, H, n_views=30)[3].to(dev)
    bg0 = torch.zeros(3, device=dev)
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg0, 1.0,
                                       cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center, False, False)
    leaves = {k: c[k].to(dev).contiguous().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    gen = torch.Generator().manual_seed(3)
    gc = synthetic.upstream_grad(H, W).to(dev)
    gd = torch.randn(1, H, W, generator=gen).to(dev)
    ga = torch.randn(1, H, W, generator=gen).to(dev)
    res = {}
    for mode in ("default", "alpha", "depth_alpha"):
        config.set_depth_gradient(mode == "depth_alpha")
        try:
            m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
            out = GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], shs=leaves["shs"],
                                         scales=leaves["scales"], rotations=leaves["rotations"], return_alpha=mode != "default")
        finally:
            config.set_depth_gradient(False)
        if mode == "default":
            outs, grads = [out[0]], [gc]
        elif mode == "alpha":
            outs, grads = [out[0], out[3]], [gc, ga]
        else:
            outs, grads = [out[0], out[2], out[3]], [gc, gd, ga]
        inputs = [m2] + list(leaves.values())

        def backward():
            torch.autograd.grad(outs, inputs, grads, retain_graph=True)
        ms = _time(backward, iters, warmup)
        _lib.profile_enable(True)
        for _ in range(iters):
            backward()
        torch.cuda.synchronize()
        st = _lib.profile_read()
        _lib.profile_enable(False)
        per = lambda k: round(st[k][0] / max(1, st[k][1]) * 1000.0, 1) if k in st and st[k][1] else None
        res[mode] = dict(backward_ms=round(ms, 4), render_bwd_us=per("render_bwd"), gauss_bwd_us=per("gauss_bwd"))
    d = res["default"]
    for mode in ("alpha", "depth_alpha"):
        x = res[mode]
        res[mode + "_over_default"] = dict(
            backward=round(x["backward_ms"] / d["backward_ms"], 3),
            render_bwd=round(x["render_bwd_us"] / d["render_bwd_us"], 3) if d["render_bwd_us"] and x["render_bwd_us"] else None)

    # the forward's alpha pass alone, on a forward's image state
    sh = leaves["shs"].detach()
    with torch.no_grad():
        fwd = _C.rasterize_gaussians(bg0, leaves["means3D"].detach(), None, leaves["opacities"].detach(),
                                     leaves["scales"].detach(), leaves["rotations"].detach(), 1.0, None,
                                     cam.world_view_transform, cam.full_proj_transform, rs.tanfovx, rs.tanfovy, H, W, sh, 3,
                                     cam.camera_center, False, False)
    img = fwd[6]
    res["alpha_kernel_us"] = round(_time(lambda: _C.render_alpha(img, H, W), iters, warmup) * 1000.0, 1)

    # the workaround: a second render with colours 1 and background 0, forward + backward of channel 0
    ones = torch.ones(P, 3, device=dev)

    def second_render():
        m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
        col = GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], colors_precomp=ones,
                                     scales=leaves["scales"], rotations=leaves["rotations"])[0]
        torch.autograd.grad([col[0:1]], [m2] + [leaves[k] for k in ("means3D", "opacities", "scales", "rotations")], [ga])
    two = _time(second_render, iters, warmup)
    added = res["alpha"]["backward_ms"] - d["backward_ms"] + res["alpha_kernel_us"] / 1000.0
    res["two_render"] = dict(second_render_fwd_bwd_ms=round(two, 4), alpha_mode_added_ms=round(added, 4))
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
    out = dict(tool="alpha_grad_bench", iters=args.iters, warmup=args.warmup, version=_lib.lib().lr_version().decode())
    for name in args.workloads.split(","):
        out[name] = run(name, args.iters, args.warmup, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
