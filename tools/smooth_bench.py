"""Cost of the fused edge-aware smoothness term against the torch composition it replaces.

    python tools/smooth_bench.py [--steps 200] [--warmup 20] [--out profiles/smooth_bench.json]

Fused: lr_smooth_forward (two launches) + lr_smooth_backward (one) on a depth map with a three-channel guide and a mask,
straight through the C ABI.  Partner: the float32 torch composition of the same definition (slices, abs, mean, exp, where,
sum; autograd backward) on the device, same tensors.  Sizes 512 x 512 and 1080p, order 1 and 2; each forward + backward pair is
timed with HIP events, the two routes ALTERNATING call by call, median of --steps after --warmup; then the fused forward and the
fused backward alone, the same way.  The bytes the algorithm needs are counted from the shapes: forward map 4 + guide 12 +
mask 4 = 20 B per pixel, backward the same 20 (weights and signs are recomputed) + gradient 4 = 24 B per pixel; neighbour reads
hit the cache.  The tensors of one size (at most 91 MB a pair) stay within the Infinity Cache between calls, so the share of the
HBM rate is the algorithmic bytes over the time, named for what it is.  Prints ONE JSON line and writes it to --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import smooth_ref as sr  # noqa: E402

HBM_ACHIEVABLE = 6.3e12             # B/s
FWD_BYTES_PER_PIXEL, BWD_BYTES_PER_PIXEL = 20, 24
GAMMA, WEIGHT = sr.GAMMA, sr.WEIGHT


def torch_smoothness(depth, guide, mask, order):
    """The definition on a depth [1,H,W] in DIRECT space with positive_only, composed from float32 torch ops."""
    H, W = depth.shape[-2:]
    valid = torch.isfinite(depth[0]) & (depth[0] > 0) & (mask > 0)
    u = torch.where(valid, depth, torch.ones_like(depth))               # no NaN may reach a product, counted or not
    total = 0.0
    for axis in (2, 1):
        n = depth.shape[axis]
        if n < order + 1:
            continue
        cut = lambda t, lo, hi, ax=axis: t.narrow(ax if t.dim() == 3 else ax - 1, lo, hi - lo)
        if order == 1:
            p, q = (0, n - 1), (1, n)
            D = cut(u, *q) - cut(u, *p)
            a = (cut(guide, *p) - cut(guide, *q)).abs().mean(dim=0)
            ok = cut(valid, *p) & cut(valid, *q)
        else:
            m, p, q = (0, n - 2), (1, n - 1), (2, n)
            D = (cut(u, *m) - 2.0 * cut(u, *p)) + cut(u, *q)
            a = torch.maximum((cut(guide, *p) - cut(guide, *m)).abs(), (cut(guide, *q) - cut(guide, *p)).abs()).mean(dim=0)
            ok = cut(valid, *m) & cut(valid, *p) & cut(valid, *q)
        w = torch.exp(-GAMMA * a)
        total = total + torch.where(ok, w * D.abs().sum(dim=0), torch.zeros_like(w)).sum()
    return total * (WEIGHT / float(H * W))


def _ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def size(H, W, order, dev, steps, warmup):
    from luciddreamer_amd import _lib
    L = _lib.lib()
    case = sr.make_case(H, W, 5, "smooth")
    d = torch.from_numpy(case["depth"][None]).to(dev)
    guide = torch.from_numpy(case["guide"]).to(dev)
    mask = torch.from_numpy(case["mask"]).to(dev)
    out = torch.empty(2, device=dev)
    grad = torch.empty_like(d)
    ws = torch.empty(int(L.lr_smooth_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    a = _lib.SmoothArgs(height=H, width=W, channels=1, guide_channels=3, map=d.data_ptr(), guide=guide.data_ptr(),
                        mask=mask.data_ptr(), order=order, space=_lib.LR_SMOOTH_DIRECT, positive_only=1, gamma=GAMMA, weight=WEIGHT,
                        out=out.data_ptr(), dL_dmap=grad.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                        stream=torch.cuda.current_stream(dev).cuda_stream)
    ref = ctypes.byref(a)

    def forward():
        assert L.lr_smooth_forward(ref) == 0

    def backward():
        assert L.lr_smooth_backward(ref) == 0

    def fused():
        forward()
        backward()

    leaf = d.clone().requires_grad_(True)

    def composition():
        leaf.grad = None
        torch_smoothness(leaf, guide, mask, order).backward()

    for _ in range(warmup):
        fused()
        composition()
    torch.cuda.synchronize()
    # the same loss and gradient from both, before any time is reported (a sanity check, not a bar: the composition's float32
    # differences may pick another sign where the double difference is within a float32 rounding of zero)
    value, g_fused = float(out[0]), grad.clone()
    want = float(torch_smoothness(leaf.detach(), guide, mask, order))
    gmax = float(leaf.grad.abs().max())
    differing = int(((g_fused - leaf.grad).abs() > 1e-5 * gmax).sum())
    assert abs(value - want) <= 1e-5 * max(1.0, abs(want)) and differing <= 1e-3 * H * W, (value, want, differing)
    ms = {"fused": [], "composition": [], "forward": [], "backward": []}
    for _ in range(steps):
        ms["fused"].append(_ms(fused))
        ms["composition"].append(_ms(composition))
    for _ in range(steps):
        ms["forward"].append(_ms(forward))
        ms["backward"].append(_ms(backward))
    med = {k: statistics.median(v) for k, v in ms.items()}
    n = H * W
    share = lambda nbytes, t_ms: round(nbytes / (t_ms * 1e-3) / HBM_ACHIEVABLE, 4)
    return {"fused_pair_us": round(med["fused"] * 1e3, 1), "composition_pair_us": round(med["composition"] * 1e3, 1),
            "composition_over_fused": round(med["composition"] / med["fused"], 2),
            "fused_min_us": round(min(ms["fused"]) * 1e3, 1), "composition_min_us": round(min(ms["composition"]) * 1e3, 1),
            "forward_us": round(med["forward"] * 1e3, 1), "backward_us": round(med["backward"] * 1e3, 1),
            "forward_bytes": FWD_BYTES_PER_PIXEL * n, "backward_bytes": BWD_BYTES_PER_PIXEL * n,
            "forward_share_of_achievable_hbm": share(FWD_BYTES_PER_PIXEL * n, med["forward"]),
            "backward_share_of_achievable_hbm": share(BWD_BYTES_PER_PIXEL * n, med["backward"]),
            "pair_share_of_achievable_hbm": share((FWD_BYTES_PER_PIXEL + BWD_BYTES_PER_PIXEL) * n, med["fused"]),
            "counted_terms": int(out[1]), "pixels_whose_gradient_differs_from_the_composition": differing}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smooth_bench: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib
    sizes = {f"{name}_order{order}": size(H, W, order, dev, args.steps, args.warmup)
             for name, (H, W) in (("512", (512, 512)), ("1080p", (1080, 1920))) for order in (1, 2)}
    res = {"tool": "smooth_bench", "steps": args.steps, "warmup": args.warmup, "version": _lib.lib().lr_version().decode(),
           "device": torch.cuda.get_device_name(0), "mode": "depth, DIRECT space, three-channel guide, mask",
           "forward_bytes_per_pixel": FWD_BYTES_PER_PIXEL, "backward_bytes_per_pixel": BWD_BYTES_PER_PIXEL,
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "timing": "HIP events around lr_smooth_forward + lr_smooth_backward, host launch included; the two routes alternate",
           "sizes": sizes}
    line = json.dumps(res, separators=(",", ":"))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
