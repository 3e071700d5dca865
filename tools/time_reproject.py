"""Cost of the point-cloud reprojection (luciddreamer_amd.reproject) at LucidDreamer's size, next to its numpy restatement.

    python tools/time_reproject.py [--size 512] [--views 8] [--frames 5] [--calls 10] [--repeats 15] [--out FILE]
    python tools/time_reproject.py --resources [--out FILE]        # no device needed

Timing (needs the MI355X): the cloud is --views synthetic RGB-D views (luciddreamer_amd.synthetic.rgbd_view) lifted at a yaw
path, 8 x 512^2 = 2 097 152 points by default, about what generate_pcd has accumulated when "Aligning" starts.  Device events
around --calls back-to-back calls, median of --repeats such windows after a warm-up: a figure is the steady-state time per call
including its allocations and the gap to the next launch.
  project_batch   --frames poses of the cloud in one call (image, masks, depth)
  masks_only      the same with image=False (no splat)
  project         one pose, with valid / pix
  lift            one depth map
  restatement     tests/reproject_ref.py project() for one pose on the host (one run, wall clock), whose every output the device's
                  frame must equal at this size too ("equal": true)
  dream           what follows the networks (csrc/dream.hip), on the first pose's frame and a miscalibrated synthetic depth map:
                  fit_scale (a, with its 32-byte read-back), correspond (b), scatter_interpolate (c) on the frame's own samples and
                  holes, dream_lift (d), compensate and dream_step as called; (c) again with 10 000 random samples on a half-empty
                  frame (the left half of the pixels are holes) and on an all-hole frame, with the float64 operation rate reached
                  (25 operations per pixel and sample); tests/dream_ref.py on the host beside each (one run, wall clock; for the
                  10 000-sample case on every 32nd hole pixel only), and whether the device's output equals it
--resources compiles csrc/reproject.hip with -Rpass-analysis=kernel-resource-usage and records registers, scratch, LDS and
occupancy per kernel; a kernel with scratch is an error.  Both modes merge their section into --out (default
profiles/reproject_timing.json), keeping the other's.
"""
import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def resources():
    from luciddreamer_amd import build
    text = ""
    for name in ("reproject.hip", "dream.hip"):
        cmd = [build.hipcc(), "-c", os.path.join(build.CSRC, name), "-o", os.devnull] + build.COMMON_FLAGS + \
              ["-I", build.OBJDIR] + build.SOURCES[name] + ["-Rpass-analysis=kernel-resource-usage"]
        text += subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "LDS Size [bytes/block]": "lds_bytes_per_block"}
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            mangled = m.group(1)
            k = re.search(r"k_(project|splat|window|resolve|lift|scale_partial|scale_final|correspond|interp|dream_lift)", mangled)
            name = k.group(0) if k else mangled
            if name == "k_window":
                name += "<dilate>" if "ILi4E" in mangled else "<erode>"
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and name and m.group(1) in keys:
            out[name][keys[m.group(1)]] = int(m.group(2))
    if not out:
        raise SystemExit("no kernel-resource-usage remarks in the compiler's output")
    bad = [k for k, v in out.items() if v.get("scratch_bytes_per_lane", 0)]
    if bad:
        raise SystemExit(f"kernels with scratch: {bad}")
    return out


def yaw_pose(angle, shift):
    import numpy as np
    c, s = math.cos(angle), math.sin(angle)
    P = np.eye(4)
    P[:3, :3] = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    P[0, 3] = shift
    return P


def timing(a):
    import numpy as np
    import torch
    from luciddreamer_amd import reproject, synthetic
    from tests import reproject_ref as RR
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_reproject.py: timing needs a HIP device (use --resources without one)")
    dev = torch.device("cuda:0")
    H = W = a.size
    focal = 0.5 * W / math.tan(math.radians(30.0))
    K = np.array([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1]])
    pts, cols = [], []
    for i in range(a.views):
        image, depth = (t.to(dev) for t in synthetic.rgbd_view(H, W, seed=i))
        P = yaw_pose(0.05 * i, -0.1 * i)
        pts.append(reproject.lift(depth, K, P[:3, :3], P[:3, 3:4]))
        cols.append(image.reshape(-1, 3))
    X, C = torch.cat(pts, dim=1).contiguous(), torch.cat(cols, dim=0).contiguous()
    N = int(X.shape[1])
    render = yaw_pose(0.05 * (a.views // 2), -0.1 * (a.views // 2))
    inner = [yaw_pose(0.0, 0.0)] + [yaw_pose(0.03 * s, 0.05 * t) for s, t in ((1, 1), (1, -1), (-1, 1), (-1, -1))]
    inner = (inner * ((a.frames + 4) // 5))[:a.frames]
    poses = [reproject.compose_pose(p[:3, :3], p[:3, 3:4], render[:3, :3], render[:3, 3:4]) for p in inner]
    Rs, Ts = np.stack([r for r, _ in poses]), np.stack([t for _, t in poses])
    depth0 = synthetic.rgbd_view(H, W)[1].to(dev)

    def window(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.calls)
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    out = {"size": [H, W], "points": N, "frames": a.frames, "calls_per_window": a.calls, "windows": a.repeats,
           "device": torch.cuda.get_device_name(0)}
    out["project_batch"] = window(lambda: reproject.project_batch(X, C, K, Rs, Ts, H, W))
    out["masks_only"] = window(lambda: reproject.project_batch(X, None, K, Rs, Ts, H, W, image=False))
    out["project"] = window(lambda: reproject.project(X, C, K, Rs[0], Ts[0], H, W))
    out["lift"] = window(lambda: reproject.lift(depth0, K, render[:3, :3], render[:3, 3:4]))
    f = reproject.project(X, C, K, Rs[0], Ts[0], H, W)
    valid = int(f.valid.sum())
    out["valid_points_frame0"] = valid
    out["mask_pixels_frame0"] = int(f.mask.sum())
    # atomics of the frame: one 4-byte minimum per valid point, 4 adds of 8 bytes per accepted neighbour with a non-zero weight
    Xh, Ch = X.cpu().numpy(), C.cpu().numpy()
    t0 = time.perf_counter()
    ref = RR.project(Xh, Ch, K, Rs[0], Ts[0], H, W)
    out["restatement_one_frame_s"] = time.perf_counter() - t0
    got = dict(image=f.image, image_u8=f.image_u8, mask=f.mask, dil=f.dilated, border=f.border, depth=f.depth, valid=f.valid,
               pix=f.pix)
    out["equal"] = all(np.array_equal(got[k].cpu().numpy(), ref[k]) for k in got)
    out["dream"] = dream_timing(window, dev, X, C, Xh, Ch, f, ref, K, Rs[0], Ts[0], H, W)
    return out


def dream_timing(window, dev, X, C, Xh, Ch, f, ref, K, R, T, H, W):
    """(a)-(d) of csrc/dream.hip on the frame `f` (restated: `ref`) of the timing run's cloud."""
    import ctypes
    import numpy as np
    import torch
    from luciddreamer_amd import _lib, reproject, synthetic
    from tests import dream_ref as DR
    L = _lib.lib()
    net = synthetic.miscalibrated_depth(synthetic.rgbd_view(H, W)[1]).to(dev)
    neth = net.cpu().numpy()
    image = (synthetic.rgbd_view(H, W)[0] * 255.0).round().to(torch.uint8).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pose = reproject._Pose(K, R, T)
    N = int(X.shape[1])
    fit = reproject.fit_scale(X, f, net, K, R, T)
    comp = reproject.compensate(X, f, net, K, R, T, scale=fit.scale)
    M = comp.n_corr
    holes = int((f.mask == 0).sum())
    d = {"n_corr": M, "hole_pixels": holes, "valid_points": int(f.valid.sum()), "scale": fit.scale, "mse_before": fit.mse_before,
         "mse_after": fit.mse_after}
    d["a_fit_scale"] = window(lambda: reproject.fit_scale(X, f, net, K, R, T))
    corr = (f.border.reshape(-1)[f.pix.clamp(min=0).long()].bool() & f.valid.bool()).nonzero()[:, 0].to(torch.int32).contiguous()
    s3 = torch.empty((3, M + 4), dtype=torch.float64, device=dev)
    common = dict(height=H, width=W, depth=net.data_ptr(), scale=fit.scale, stream=stream, **pose.fields())
    ca = _lib.DreamArgs(n_points=N, points=X.data_ptr(), point_stride=1, coord_stride=N, pix=f.pix.data_ptr(),
                        corr=corr.data_ptr() if M else None, n_corr=M, out_su=s3[0].data_ptr(), out_sv=s3[1].data_ptr(),
                        out_sval=s3[2].data_ptr(), **common)
    d["b_correspond"] = window(lambda: L.lr_dream_correspond(ctypes.byref(ca)))
    uv, val = comp.corr_uv.contiguous(), comp.corr_value.contiguous()
    d["c_scatter_interpolate"] = window(lambda: reproject.scatter_interpolate(uv, val, H, W, f.mask))
    lifted = torch.empty((3, H * W), dtype=torch.float32, device=dev)
    la = _lib.DreamArgs(new_depth=comp.new_depth.data_ptr(), out_points=lifted.data_ptr(), **common)
    d["d_dream_lift"] = window(lambda: L.lr_dream_lift(ctypes.byref(la)))
    d["compensate"] = window(lambda: reproject.compensate(X, f, net, K, R, T, scale=fit.scale))
    d["dream_step"] = window(lambda: reproject.dream_step(X, C, f, image, net, K, R, T))
    # the host restatement of the same call, and equality
    t0 = time.perf_counter()
    want_p, want_c, info = DR.dream_step(Xh, Ch, ref, image.cpu().numpy(), neth, K, R, T, H, W, "lstsq")
    d["restatement_dream_step_s"] = time.perf_counter() - t0
    pts, cols, got = reproject.dream_step(X, C, f, image, net, K, R, T)
    d["equal"] = bool(np.array_equal(pts.cpu().numpy(), want_p) and np.array_equal(cols.cpu().numpy(), want_c) and
                      got.scale == info["scale"] and np.array_equal(comp.new_depth.cpu().numpy(), info["comp"]["new_depth"]))
    # (c) at the size the kernel is built for: 10 000 samples, half of the frame / all of it to fill
    rng = np.random.default_rng(1)
    Ms = 10_000
    su, sv, sv_ = rng.uniform(0, W - 1, Ms), rng.uniform(0, H - 1, Ms), rng.uniform(-0.5, 0.5, Ms)
    uvd = torch.from_numpy(np.stack([su, sv], axis=1)).to(dev)
    vald = torch.from_numpy(sv_).to(dev)
    for name, where in (("half_empty", np.tile((np.arange(W) >= W // 2).astype(np.uint8), (H, 1))),
                        ("all_holes", np.zeros((H, W), dtype=np.uint8))):
        wd = torch.from_numpy(where).to(dev)
        r = window(lambda: reproject.scatter_interpolate(uvd, vald, H, W, wd))
        q = int((where == 0).sum())
        r["samples"], r["hole_pixels"] = Ms, q
        r["float64_gops_per_s"] = 25.0 * q * Ms / (r["median_ms"] * 1e-3) / 1e9
        sub = np.full((H, W), 1, dtype=np.uint8)
        sub.reshape(-1)[np.nonzero(where.reshape(-1) == 0)[0][::32]] = 0
        t0 = time.perf_counter()
        host = DR.scatter(su, sv, sv_, H, W, sub)
        r["restatement_every_32nd_hole_s"] = time.perf_counter() - t0
        g = reproject.scatter_interpolate(uvd, vald, H, W, wd).cpu().numpy()
        r["equal_on_those"] = bool(np.array_equal(g[sub == 0], host[sub == 0]))
        d["c_10000_samples_" + name] = r
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_timing.json"))
    a = ap.parse_args()
    data = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            data = json.load(f)
    data["tool"] = "tools/time_reproject.py"
    if a.resources:
        data["kernel_resources"] = resources()
    else:
        data["timing"] = timing(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print(json.dumps(data["kernel_resources" if a.resources else "timing"], indent=1))
    if not a.resources and not data["timing"]["equal"]:
        raise SystemExit("the device's frame differs from the restatement")
    if not a.resources and not data["timing"]["dream"]["equal"]:
        raise SystemExit("the device's dream step differs from the restatement")


if __name__ == "__main__":
    main()
