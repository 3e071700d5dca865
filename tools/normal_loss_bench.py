"""Cost of the fused normal loss against the torch composition it replaces.

    python tools/normal_loss_bench.py [--steps 200] [--warmup 20] [--out profiles/normal_loss_bench.json]

Fused: lr_normal_loss_forward (two launches) + lr_normal_loss_backward (one), target-normal mode without a weight plane, straight
through the C ABI.  Partner: the float32 torch composition of the tests' reference (tests/normal_ref.torch_loss: lifted points,
torch.cross, autograd backward) on the device, same inputs.  Sizes 1080p and 512 x 512; each forward + backward pair is timed
with HIP events, the two ALTERNATING call by call, median of --steps after --warmup.  The bytes the algorithm needs are counted
from the shapes: forward depth 4 + target 12, backward depth 4 + target 12 + gradient 4 = 36 B per pixel (the backward recomputes
the normals, so it reads the target again; neighbour reads hit the cache).  Prints ONE JSON line and writes it to --out.
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

from tests import normal_ref as nr  # noqa: E402

HBM_ACHIEVABLE = 6.3e12             # B/s
BYTES_PER_PIXEL = 36


def _pair_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def size(H, W, dev, steps, warmup):
    from luciddreamer_amd import _lib
    L = _lib.lib()
    case = nr.make_case(H, W, 5, "smooth")
    d = torch.from_numpy(case["depth"]).to(dev)
    t = torch.from_numpy(case["target_normals"]).to(dev)
    out = torch.empty(2, device=dev)
    grad = torch.empty_like(d)
    ws = torch.empty(int(L.lr_normals_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    tx, ty = nr.TAN
    a = _lib.NormalsArgs(height=H, width=W, tan_fovx=tx, tan_fovy=ty, depth=d.data_ptr(), target_normals=t.data_ptr(), weight=1.0,
                         out=out.data_ptr(), dL_ddepth=grad.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                         stream=torch.cuda.current_stream(dev).cuda_stream)
    ref = ctypes.byref(a)

    def fused():
        assert L.lr_normal_loss_forward(ref) == 0 and L.lr_normal_loss_backward(ref) == 0

    leaf = d.clone().requires_grad_(True)

    def composition():
        leaf.grad = None
        nr.torch_loss(leaf, tx, ty, target_normals=t)[0].backward()

    for _ in range(warmup):
        fused()
        composition()
    torch.cuda.synchronize()
    # the same loss from both, before any time is reported
    value, g_fused = float(out[0]), grad.clone()
    composition()
    torch.cuda.synchronize()
    want = float(nr.torch_loss(leaf.detach(), tx, ty, target_normals=t)[0])
    gmax = float(leaf.grad.abs().max())
    # (a sanity check, not a bar: the float32 lifted-point composition loses digits with the resolution)
    assert abs(value - want) <= 1e-4 and float((g_fused - leaf.grad).abs().max()) <= 2e-2 * gmax, (value, want)
    ms = {"fused": [], "composition": []}
    for _ in range(steps):
        ms["fused"].append(_pair_ms(fused))
        ms["composition"].append(_pair_ms(composition))
    f, c = statistics.median(ms["fused"]), statistics.median(ms["composition"])
    n_bytes = BYTES_PER_PIXEL * H * W
    return {"fused_pair_us": round(f * 1e3, 1), "composition_pair_us": round(c * 1e3, 1), "composition_over_fused": round(c / f, 2),
            "fused_min_us": round(min(ms["fused"]) * 1e3, 1), "composition_min_us": round(min(ms["composition"]) * 1e3, 1),
            "bytes_needed": n_bytes, "fused_bytes_per_s": round(n_bytes / (f * 1e-3), 0),
            "share_of_achievable_hbm": round(n_bytes / (f * 1e-3) / HBM_ACHIEVABLE, 4), "counted": int(out[1])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normal_loss_bench: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib
    res = {"tool": "normal_loss_bench", "steps": args.steps, "warmup": args.warmup, "version": _lib.lib().lr_version().decode(),
           "device": torch.cuda.get_device_name(0), "mode": "target normals, no weight plane", "bytes_per_pixel": BYTES_PER_PIXEL,
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "timing": "HIP events around lr_normal_loss_forward + _backward, host launch included",
           "sizes": {"1080p": size(1080, 1920, dev, args.steps, args.warmup), "512": size(512, 512, dev, args.steps, args.warmup)}}
    line = json.dumps(res, separators=(",", ":"))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
