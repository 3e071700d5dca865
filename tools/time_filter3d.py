"""Cost of the 3D smoothing filter (luciddreamer_amd.filter3d) against what a user composes from torch ops today.

    python tools/time_filter3d.py [--gaussians 1000000] [--cameras 30] [--calls 20] [--repeats 30] [--rounds 3] [--out FILE]
    python tools/time_filter3d.py --resources [--out FILE]        # no device needed

Timing (needs the MI355X): device events around --calls back-to-back calls, median of --repeats such windows after a warm-up, so
that a figure is the steady-state time per call including the gap to the next launch.
  kernels   lr_filter3d_apply_forward / _backward in each domain and lr_filter3d_update through the C ABI, with the bytes/s they
            achieve on the algorithmic bytes (36 / 52 / 16 B per Gaussian) next to the 6.29 TB/s a float4 copy reaches on this chip.
  pair      filter3d.apply + autograd backward against the torch-op composition of the same function (exp, square, prod, sqrt,
            sigmoid, log and their autograd nodes), fused and composed alternating for --rounds rounds in the same process; the
            fused pair must not be slower (exit status 1 and "fused_not_slower": false otherwise).
  update    compute_filter_3d against the Python loop over the cameras.
--resources compiles csrc/filter3d.hip with -Rpass-analysis=kernel-resource-usage and records VGPRs, SGPRs, scratch, LDS and
occupancy per kernel; a kernel with scratch is an error.  Both modes merge their section into --out (default
profiles/filter3d_timing.json), keeping the other's.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_TBPS = 6.29                    # measured float4 streaming copy of the MI355X (8.0 TB/s HBM3E peak)
BYTES = {"apply_forward": 36, "apply_backward": 52, "update": 16}


def resources():
    from luciddreamer_amd import build
    src = os.path.join(build.CSRC, "filter3d.hip")
    cmd = [build.hipcc(), "-c", src, "-o", os.devnull] + build.COMMON_FLAGS + ["-I", build.OBJDIR] + build.SOURCES["filter3d.hip"] + \
          ["-Rpass-analysis=kernel-resource-usage"]
    os.makedirs(build.OBJDIR, exist_ok=True)
    build._write_hash_header()
    text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "LDS Size [bytes/block]": "lds_bytes_per_block"}
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            mangled = m.group(1)
            k = re.search(r"k_filter3d_[a-z_]+?(?=E|I)", mangled)
            name = k.group(0) if k else mangled
            if "ILb1E" in mangled:
                name += "<activated>"
            elif "ILb0E" in mangled:
                name += "<stored>"
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and name and m.group(1) in keys:
            out[name][keys[m.group(1)]] = int(m.group(2))
    if not out:
        raise RuntimeError("no kernel-resource-usage remarks in the compiler's output")
    spilling = [k for k, v in out.items() if v.get("scratch_bytes_per_lane", 0) != 0]
    if spilling:
        raise RuntimeError(f"kernels with scratch: {spilling}")
    return out


def window(fn, calls, repeats, warmup=3):
    """Median over `repeats` windows of `calls` back-to-back calls, in microseconds per call."""
    import torch
    for _ in range(warmup * calls):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return statistics.median(out)


def torch_apply(r, q, f, activated):
    """What a user writes today (Mip-Splatting's get_scaling_with_3D_filter / get_opacity_with_3D_filter, and their logs for the
    stored domain)."""
    import torch
    s2 = torch.square(torch.exp(r))
    s2f = s2 + torch.square(f)
    coef = torch.sqrt(s2.prod(dim=1, keepdim=True) / s2f.prod(dim=1, keepdim=True))
    o = torch.sigmoid(q) * coef
    s = torch.sqrt(s2f)
    if activated:
        return s, o
    return torch.log(s), torch.log(o / (1 - o))


def torch_update(xyz, packed, variance=0.2):
    """The Python loop over the cameras (the shape of Mip-Splatting's compute_3D_filter, with the paper's min of z / fx)."""
    import torch
    P = xyz.shape[0]
    d = torch.full((P,), float("inf"), device=xyz.device)
    ones = torch.ones((P, 1), device=xyz.device)
    h = torch.cat((xyz, ones), dim=1)
    for n in range(packed.shape[0]):
        c = packed[n]
        v = h @ c[:16].reshape(4, 4)
        z = v[:, 2]
        ok = (z > 0.2) & ((v[:, 0] / z * c[16]).abs() <= 0.65 * c[18]) & ((v[:, 1] / z * c[17]).abs() <= 0.65 * c[19])
        d = torch.where(ok, torch.minimum(d, z / c[16]), d)
    seen = torch.isfinite(d)
    widest = torch.where(seen, d, torch.zeros_like(d)).max()
    return (variance ** 0.5 * torch.where(seen, d, widest))[:, None]


def timing(args):
    import torch
    from luciddreamer_amd import _lib, cameras, filter3d
    if not torch.cuda.is_available():
        raise RuntimeError("tools/time_filter3d.py: no HIP device (timings are taken on the MI355X only)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    P, V = args.gaussians, args.cameras
    g = torch.Generator().manual_seed(0)
    r = (torch.rand(P, 3, generator=g) * 6 - 7).to(dev)                       # scales e^-7 .. e^-1
    q = (torch.rand(P, 1, generator=g) * 8 - 4).to(dev)
    xyz = (torch.rand(P, 3, generator=g) * torch.tensor([6.0, 6.0, 7.0]) + torch.tensor([-3.0, -3.0, -1.0])).to(dev)
    packed = filter3d.pack_cameras(cameras.lookaround_path(1920, 1080, n_views=V), dev)
    f = filter3d.compute_filter_3d(xyz, packed)
    gs, go = torch.randn(P, 3, generator=g).to(dev), torch.randn(P, 1, generator=g).to(dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    out_s, out_o = torch.empty_like(r), torch.empty_like(q)
    ws = torch.empty(int(L.lr_filter3d_workspace_bytes(P)), dtype=torch.uint8, device=dev)
    fo = torch.empty_like(f)
    res = {"gaussians": P, "cameras": V, "calls_per_window": args.calls, "windows": args.repeats, "rounds": args.rounds,
           "version": L.lr_version().decode(), "device": torch.cuda.get_device_name(0), "copy_tbps_reference": COPY_TBPS}

    def rate(us, what):
        tbps = BYTES[what] * P / (us * 1e-6) / 1e12
        return {"us": round(us, 2), "tbps": round(tbps, 3), "fraction_of_copy": round(tbps / COPY_TBPS, 3)}
    kernels = {}
    for act, dom in ((0, "stored"), (1, "activated")):
        fwd = lambda: L.lr_filter3d_apply_forward(P, r.data_ptr(), q.data_ptr(), f.data_ptr(), act, out_s.data_ptr(), out_o.data_ptr(), s)
        bwd = lambda: L.lr_filter3d_apply_backward(P, r.data_ptr(), q.data_ptr(), f.data_ptr(), act, gs.data_ptr(), go.data_ptr(),
                                                   out_s.data_ptr(), out_o.data_ptr(), s)
        assert fwd() == 0 and bwd() == 0
        kernels[f"apply_forward_{dom}"] = rate(window(fwd, args.calls, args.repeats), "apply_forward")
        kernels[f"apply_backward_{dom}"] = rate(window(bwd, args.calls, args.repeats), "apply_backward")
    upd = lambda: L.lr_filter3d_update(P, V, xyz.data_ptr(), packed.data_ptr(), 0.2, fo.data_ptr(), None, ws.data_ptr(), s)
    assert upd() == 0
    kernels["update"] = rate(window(upd, args.calls, args.repeats), "update")
    res["kernels"] = kernels

    # the pair through autograd against the composition, alternating
    rp, qp = r.clone().requires_grad_(True), q.clone().requires_grad_(True)

    def pair(fn, act):
        def run():
            rp.grad = qp.grad = None
            so, oo = fn(rp, qp, f, act)
            torch.autograd.backward([so, oo], [gs, go])
        return run
    pairs, ok = {}, True
    for act, dom in ((False, "stored"), (True, "activated")):
        fused, composed = [], []
        for _ in range(args.rounds):
            fused.append(window(pair(lambda a, b, c, d: filter3d.apply(a, b, c, activated=d), act), args.calls, args.repeats))
            composed.append(window(pair(torch_apply, act), args.calls, args.repeats))
        fu, co = statistics.median(fused), statistics.median(composed)
        pairs[dom] = {"fused_us": round(fu, 2), "torch_ops_us": round(co, 2), "torch_over_fused": round(co / fu, 2),
                      "fused_rounds_us": [round(x, 2) for x in fused], "torch_rounds_us": [round(x, 2) for x in composed]}
        ok = ok and fu <= co
    res["forward_plus_backward"] = pairs
    fused, looped = [], []
    for _ in range(args.rounds):
        fused.append(window(lambda: filter3d.compute_filter_3d(xyz, packed), args.calls, args.repeats))
        looped.append(window(lambda: torch_update(xyz, packed), max(1, args.calls // 10), max(3, args.repeats // 3), warmup=1))
    fu, co = statistics.median(fused), statistics.median(looped)
    res["update_against_the_camera_loop"] = {"fused_us": round(fu, 2), "torch_loop_us": round(co, 2), "torch_over_fused": round(co / fu, 2)}
    a, b = torch_update(xyz, packed), filter3d.compute_filter_3d(xyz, packed)
    # the loop forms the view-space position by a matrix product, in another order: a pair at the edge of a test may fall elsewhere
    res["update_against_the_camera_loop"]["rows_differing_by_more_than_1e-5_relative"] = int(((a - b).abs() > 1e-5 * b.abs()).sum())
    res["fused_not_slower"] = bool(ok and fu <= co)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--cameras", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter3d_timing.json"))
    args = ap.parse_args()
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc["tool"] = "tools/time_filter3d.py"
    if args.resources:
        doc["kernel_resources"] = resources()
    else:
        doc["timing"] = timing(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc, separators=(",", ":")))
    if not args.resources and not doc["timing"]["fused_not_slower"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
