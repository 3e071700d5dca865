"""Cost of the N-channel feature map pass (lr_render_features) and of its backward (lr_render_features_backward) against the
workaround it replaces -- ceil(C/3) colour renders with colors_precomp = three columns of the table -- and against the rendered
normal map pass, the 3-channel yardstick, on the same view.

    python tools/feature_bench.py [--iters 25] [--warmup 5] [--workloads c3,ld512] [--channels 16,32] [--view 0]

For each workload (bench.py's C3 and LD-512 clouds and cameras, one view of the rotate360 path) one exact-mode forward is run
through the binding; on its buffers the feature pass and its whole backward are timed for every channel count with HIP events
around ten calls back to back (per call; median of --iters after --warmup).  The library's per-stage events give, over --iters
feature backwards, the per-tile stage (k_features_bwd with the zero-fill of dL_dfeatures and k_feature_rows, once per 16 channels;
recorded as that call's render_bwd stage) and the per-Gaussian stage behind it (k_gauss_bwd, once per call; gauss_bwd).  In the
same process the workaround is timed on the same view the same way: its ceil(C/3) exact-mode colour forwards (preprocess, binning
and blend each, with the read-back exact mode needs), and its ceil(C/3) colour backwards on those forwards' buffers, gradients
accumulated in place; and so is the normal pass.  Prints ONE JSON line; times in microseconds, ratios workaround / feature pass.
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


def run(name, view, iters, warmup, channels, dev):
    from types import SimpleNamespace
    from luciddreamer_amd import _C, _lib, cameras, synthetic
    kind, P, (W, H) = WORKLOADS[name]
    c = {k: v.to(dev).contiguous() for k, v in synthetic.make_cloud(P, kind, 0).items()}
    cam = cameras.rotate360_path(W, H, n_views=30)[view].to(dev)
    bg = torch.zeros(3, device=dev)
    tfx, tfy = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    rs = SimpleNamespace(image_height=H, image_width=W, tanfovx=tfx, tanfovy=tfy, scale_modifier=1.0,
                         viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center)

    def forward(colors=None):
        return _C.rasterize_gaussians(bg, c["means3D"], colors, c["opacities"], c["scales"], c["rotations"], 1.0, None,
                                      cam.world_view_transform, cam.full_proj_transform, tfx, tfy, H, W,
                                      c["shs"] if colors is None else None, 3, cam.camera_center, False, False)
    R, color, depth, radii, geom, binning, img = forward()
    inputs = dict(means3D=c["means3D"], scales=c["scales"], rotations=c["rotations"])
    acc = dict(means2D=torch.zeros(P, 3, device=dev), opacity=torch.zeros(P, 1, device=dev), means3D=torch.zeros(P, 3, device=dev),
               scales=torch.zeros(P, 3, device=dev), rotations=torch.zeros(P, 4, device=dev))
    gen = torch.Generator().manual_seed(3)
    empty = torch.Tensor([])

    normals, gauss_normals = _C.render_normals(geom, binning, img, radii, rs, **inputs)
    gn = torch.randn(3, H, W, generator=gen).to(dev)
    out = dict(instances=int(R),
               normals_fwd_us=_time_us(lambda: _C.render_normals(geom, binning, img, radii, rs, **inputs), iters, warmup),
               normals_backward_us=_time_us(lambda: _C.render_normals_backward(geom, binning, img, gn, normals, gauss_normals, radii,
                                                                               rs, accumulate_into=acc, **inputs), iters, warmup))
    for C in channels:
        table = (2.0 * torch.rand(P, C, generator=gen) - 1.0).to(dev)
        G = torch.randn(C, H, W, generator=gen).to(dev)
        F = _C.render_features(geom, binning, img, table, rs)
        acc_f = dict(acc, features=torch.zeros(P, C, device=dev))

        def features_backward():
            _C.render_features_backward(geom, binning, img, G, F, table, radii, rs, slots=int(R), accumulate_into=acc_f, **inputs)
        per = _stages(features_backward, iters)
        fwd = _time_us(lambda: _C.render_features(geom, binning, img, table, rs), iters, warmup)
        bwd = _time_us(features_backward, iters, warmup)
        # the workaround: one colour render per three channels (the last group zero-padded), each with a backward of its own
        groups = []
        for k in range(0, C, 3):
            cols = torch.zeros(P, 3, device=dev)
            cols[:, :min(3, C - k)] = table[:, k:k + 3]
            g3 = torch.zeros(3, H, W, device=dev)
            g3[:min(3, C - k)] = G[k:k + 3]
            groups.append((cols, g3))
        states = [forward(cols) for cols, _ in groups]
        acc_w = dict(acc, colors=torch.zeros(P, 3, device=dev))

        def workaround_forward():
            for cols, _ in groups:
                forward(cols)

        def workaround_backward():
            for (cols, g3), (R_, _, _, radii_, geom_, binning_, img_) in zip(groups, states):
                _C.rasterize_gaussians_backward(bg, c["means3D"], radii_, cols, c["scales"], c["rotations"], 1.0, empty,
                                                cam.world_view_transform, cam.full_proj_transform, tfx, tfy, g3, None, empty, 3,
                                                cam.camera_center, geom_, R_, binning_, img_, False, accumulate_into=acc_w,
                                                skip_unused=True)
        w_fwd = _time_us(workaround_forward, iters, warmup)
        w_bwd = _time_us(workaround_backward, iters, warmup)
        del states
        out["C%d" % C] = dict(features_fwd_us=fwd, features_backward_us=bwd, k_features_bwd_stage_us=per("render_bwd"),
                              gauss_stage_us=per("gauss_bwd"), renders_of_the_workaround=len(groups),
                              workaround_fwd_us=w_fwd, workaround_backward_us=w_bwd,
                              fwd_ratio=round(w_fwd / fwd, 2), backward_ratio=round(w_bwd / bwd, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default="c3,ld512")
    ap.add_argument("--channels", default="16,32")
    ap.add_argument("--view", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib
    out = dict(tool="feature_bench", iters=args.iters, warmup=args.warmup, view=args.view, chunk=_lib.LR_FEATURE_CHUNK,
               version=_lib.lib().lr_version().decode())
    for name in args.workloads.split(","):
        out[name] = run(name, args.view, args.iters, args.warmup, [int(v) for v in args.channels.split(",")], dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
