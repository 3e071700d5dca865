"""Cost of the fused geometry pass (lr_render_geometry / lr_geometry_backward) beside the two passes it replaces in the multi-view
step (lr_render_distortion + lr_render_normals, lr_distortion_backward + lr_render_normals_backward), and of the two terms in a step.

    python tools/geom_bench.py [--iters 25] [--warmup 5] [--workloads c3,ld512] [--view 0] [--map ndc] [--step-views 6]
                               [--out profiles/geom_bench.json]

For each workload (bench.py's C3 and LD-512 clouds and cameras, one view of the rotate360 path) one exact-mode forward is run
through the binding.  On its buffers the fused and the separate forms are timed in ONE process with HIP events around ten calls
back to back (per call), --iters rounds after --warmup, the two forms ALTERNATING within each round so that a drift of the clock
hits both alike; median, minimum and the interquartile range of each are reported, and the verdict of the keep rule: fused below
the separate pair by more than the runs' own spread (the larger of the two interquartile ranges), each direction.  The backward
forms are timed as the step calls them: accumulate mode, both upstreams.  The per-tile kernels alone come from the library's stage
events (k_geom_bwd against k_distort_bwd + k_normals_bwd).
`step`: a C3-sized training step (parallel.ViewBatch with targets, --step-views views, 3 chains) with both terms against the same
step without them, alternating, per step and per view.  Prints ONE JSON line and writes it to --out; times in microseconds.
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


def _interval_us(fn, inner=INNER):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):                      # back to back: the interval is the kernels', not one call's host time
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / inner


def _alternate(forms, iters, warmup, inner=INNER):
    """{name: dict(median, min, iqr)} of the callables in `forms`, timed in alternation: one interval of each per round."""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(iters):
        for k, fn in forms.items():
            times[k].append(_interval_us(fn, inner))
    out = {}
    for k, t in times.items():
        q = statistics.quantiles(t, n=4)
        out[k] = dict(median=round(statistics.median(t), 1), min=round(min(t), 1), iqr=round(q[2] - q[0], 1))
    return out


def _verdict(pair):
    """fused below separate by more than the runs' own spread?"""
    gain = pair["separate"]["median"] - pair["fused"]["median"]
    spread = max(pair["separate"]["iqr"], pair["fused"]["iqr"])
    return dict(gain_us=round(gain, 1), spread_us=round(spread, 1), fused_over_separate=round(pair["fused"]["median"] / pair["separate"]["median"], 3),
                keep=bool(gain > spread))


def _stages(fn, iters):
    """stage -> microseconds per call of `fn` (a form that makes two calls of the library has both in its figure)."""
    from luciddreamer_amd import _lib
    _lib.profile_enable(True)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    st = _lib.profile_read()
    _lib.profile_enable(False)
    return lambda k: round(st[k][0] / iters * 1000.0, 1) if k in st and st[k][1] else None


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
    R, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
        bg, c["means3D"], None, c["opacities"], c["scales"], c["rotations"], 1.0, None, cam.world_view_transform,
        cam.full_proj_transform, tfx, tfy, H, W, c["shs"], 3, cam.camera_center, False, False)
    inputs = dict(means3D=c["means3D"], scales=c["scales"], rotations=c["rotations"])

    def fwd_separate():
        _C.render_distortion(geom, binning, img, P, H, W, distortion_map=mapping)
        _C.render_normals(geom, binning, img, radii, rs, **inputs)

    def fwd_fused():
        _C.render_geometry(geom, binning, img, radii, rs, distortion_map=mapping, **inputs)
    dist, mom, nrm, gn = _C.render_geometry(geom, binning, img, radii, rs, distortion_map=mapping, **inputs)
    d1, m1 = _C.render_distortion(geom, binning, img, P, H, W, distortion_map=mapping)
    n1, _ = _C.render_normals(geom, binning, img, radii, rs, **inputs)
    same = bool(torch.equal(dist, d1) and torch.equal(mom, m1) and torch.equal(nrm, n1))
    gen = torch.Generator().manual_seed(3)
    gd = torch.randn(1, H, W, generator=gen).to(dev)
    gnrm = torch.randn(3, H, W, generator=gen).to(dev)
    acc = dict(means2D=torch.zeros(P, 3, device=dev), opacity=torch.zeros(P, 1, device=dev), means3D=torch.zeros(P, 3, device=dev),
               scales=torch.zeros(P, 3, device=dev), rotations=torch.zeros(P, 4, device=dev))

    def bwd_separate():
        _C.distortion_backward(geom, binning, img, gd, dist, mom, rs, distortion_map=mapping, accumulate_into=acc, **inputs)
        _C.render_normals_backward(geom, binning, img, gnrm, nrm, gn, radii, rs, accumulate_into=acc, **inputs)

    def bwd_fused():
        _C.geometry_backward(geom, binning, img, gd, dist, mom, gnrm, nrm, gn, radii, rs, distortion_map=mapping, accumulate_into=acc,
                             **inputs)
    # the gradients agree (both forms from zeroed accumulators), at the sizes that are timed
    agree = {}
    for k in acc:
        acc[k].zero_()
    bwd_separate()
    want = {k: v.clone() for k, v in acc.items()}
    for k in acc:
        acc[k].zero_()
    bwd_fused()
    for k in acc:
        agree[k] = float((acc[k] - want[k]).abs().max() / want[k].abs().max())
    fwd = _alternate(dict(separate=fwd_separate, fused=fwd_fused), iters, warmup)
    bwd = _alternate(dict(separate=bwd_separate, fused=bwd_fused), iters, warmup)
    per_s, per_f = _stages(bwd_separate, iters), _stages(bwd_fused, iters)
    return dict(instances=int(R), forward_outputs_equal=same, backward_max_rel_diff=max(agree.values()),
                forward=fwd, forward_verdict=_verdict(fwd), backward=bwd, backward_verdict=_verdict(bwd),
                tile_kernels_separate_us=per_s("render_bwd"), tile_kernel_fused_us=per_f("render_bwd"),
                gauss_stage_separate_us=per_s("gauss_bwd"), gauss_stage_fused_us=per_f("gauss_bwd"),
                fwd_shape=_lib.last_launch_shapes()[0])


def step_cost(views, iters, warmup, mapping, dev):
    """A C3-sized training step with both terms against the same step without them (per step, ms; per view, us)."""
    from luciddreamer_amd import cameras, parallel, synthetic
    from tools.views_depth_bench import capacity
    kind, P, (W, H) = WORKLOADS["c3"]
    c = {k: v.to(dev).contiguous() for k, v in synthetic.make_cloud(P, kind, 0).items()}
    cams = [cc.to(dev) for cc in cameras.rotate360_path(W, H, n_views=30)[:views]]
    bg = torch.zeros(3, device=dev)
    cap = capacity(c, cams, bg, W, H)
    gen = torch.Generator().manual_seed(3)
    targets = [torch.rand(3, H, W, generator=gen).to(dev) for _ in cams]
    acc = {"means3D": torch.zeros(P, 3, device=dev), "means2D": torch.zeros(P, 3, device=dev),
           "opacity": torch.zeros(P, 1, device=dev), "sh": torch.zeros_like(c["shs"]), "scales": torch.zeros(P, 3, device=dev),
           "rotations": torch.zeros(P, 4, device=dev)}
    plain = parallel.ViewBatch(cams, None, 3, bg, cap, n_streams=3, targets=targets)
    terms = parallel.ViewBatch(cams, None, 3, bg, cap, n_streams=3, targets=targets, distortion_weight=100.0, distortion_map=mapping,
                               normal_consistency_weight=0.05)
    run_of = lambda b: (lambda: b.run(c["means3D"], c["opacities"], c["scales"], c["rotations"], c["shs"], acc))
    t = _alternate(dict(without=run_of(plain), with_terms=run_of(terms)), iters, warmup, inner=1)
    plain.check()
    terms.check()
    extra = t["with_terms"]["median"] - t["without"]["median"]
    return dict(views=views, streams=3, capacity=cap, step_us=t, extra_per_step_us=round(extra, 1),
                extra_per_view_us=round(extra / views, 1), ratio=round(t["with_terms"]["median"] / t["without"]["median"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default="c3,ld512")
    ap.add_argument("--view", type=int, default=0)
    ap.add_argument("--map", default="ndc", choices=("ndc", "linear"))
    ap.add_argument("--step-views", type=int, default=6, help="0: no step measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geom_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib
    out = dict(tool="geom_bench", iters=args.iters, warmup=args.warmup, view=args.view, map=args.map, inner=INNER,
               version=_lib.lib().lr_version().decode())
    for name in args.workloads.split(","):
        out[name] = run(name, args.view, args.iters, args.warmup, args.map, dev)
        torch.cuda.empty_cache()
    if args.step_views > 0:
        out["step"] = step_cost(args.step_views, args.iters, args.warmup, args.map, dev)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
