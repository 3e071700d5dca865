#!/usr/bin/env python
"""Generates tests/golden/ref_video_fixtures.npz by running the reference's OWN post-processing of render_video
(/root/reference/luciddreamer.py:250-265): its frame expression and utils.depth.colorize (/root/reference/utils/depth.py,
matplotlib's jet), on CPU.  Only the build container can run this (it needs the reference and matplotlib); the fixtures travel.

    python tests/golden/make_video_fixtures.py

Keys: d_<case> (float32 [1,H,W], a rendered depth), rgba_<case> (uint8 [H,W,4]), vmm_<case> (float32 [2]: the percentiles
colorize used); img_<case> (float32 [3,H,W]), u8_<case> (uint8 [H,W,3]); lut_jet (uint8 [259,4], matplotlib's jet._lut as
bytes); for the 512 x 512 cases (inputs: tests/video_ref.py big_depth_cases / big_image_cases) sha_rgba_<case>, sha_u8_<case>
(SHA-256 of the output bytes) and vmm_<case> instead.  No depth case without a valid pixel: there the reference raises IndexError (the product's documented difference);
no 1x1 depth case: colorize squeezes it to a 0-d array and fails on item assignment (the 1x1 frame case is here).
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import video_ref                                   # noqa: E402  (the 512 x 512 inputs and the frame specials)


def depth_cases():
    r = np.random.default_rng(2024)
    c = {}

    def rand(H, W, lo=0.5, hi=8.0):
        return r.uniform(lo, hi, (1, H, W)).astype(np.float32)

    c["two_1x2"] = rand(1, 2)
    c["rand_17x5"] = rand(17, 5)
    d = rand(64, 96)
    d[:, :10] = 0.0                                         # background: -0.0 after the negation
    d[:, 10:14] = -1.5                                      # negative depth: -0.0 too
    c["rand_64x96"] = d
    c["ties_64x96"] = r.choice(np.array([0.0, 1.0, 2.5, 2.5, 3.0, 7.25], np.float32), (1, 64, 96))
    c["two_values_17x5"] = r.choice(np.array([1.0, 4.0], np.float32), (1, 17, 5))
    c["const_64x96"] = np.full((1, 64, 96), 3.25, np.float32)                     # vmin == vmax
    c["zeros_17x5"] = np.zeros((1, 17, 5), np.float32)                            # all -0.0: vmin == vmax == 0
    d = rand(64, 96)
    d[0, ::3, ::2] = 99.0                                   # v == -99 exactly: invalid pixels (background colour)
    c["invalid_64x96"] = d
    d = rand(17, 5)
    d[0, 3, 2] = np.nan                                     # a NaN among the valid values: vmin = vmax = NaN
    c["nan_17x5"] = d
    return c


def image_cases():
    r = np.random.default_rng(7)
    c = {}
    special = video_ref.frame_specials()        # k + 0.5 ties after the float32 multiply by 255, 1 - ulp, 0 / 1, < 0, > 1
    for name, (H, W) in {"one_1x1": (1, 1), "two_1x2": (1, 2), "rand_17x5": (17, 5), "rand_64x96": (64, 96)}.items():
        x = r.uniform(-0.2, 1.2, (3, H, W)).astype(np.float32)
        flat = x.reshape(-1)
        k = min(flat.size // 2, special.size)
        flat[:k] = special[:k]
        r.shuffle(flat)
        c[name] = flat.reshape(3, H, W)
    return c


def main():
    sys.path.insert(0, REF)
    from utils.depth import colorize                         # reference code
    import matplotlib

    def depth_ref(d):
        depth = torch.from_numpy(d)
        value = -(depth * (depth > 0)).detach().cpu().numpy()      # luciddreamer.py:257
        rgba = colorize(value)                                      # luciddreamer.py:265
        v = value.squeeze()
        mask = v != -99
        with np.errstate(invalid="ignore"):
            vmm = np.array([np.percentile(v[mask], 2), np.percentile(v[mask], 98)], np.float32)
        return np.ascontiguousarray(rgba), vmm

    def frame_ref(x):
        frame = torch.from_numpy(x)
        return np.round(frame.permute(1, 2, 0).detach().cpu().numpy().clip(0, 1) * 255.).astype(np.uint8)   # luciddreamer.py:254-255

    out = {}
    for name, d in depth_cases().items():
        out["d_" + name] = d
        out["rgba_" + name], out["vmm_" + name] = depth_ref(d)
    for name, x in image_cases().items():
        out["img_" + name], out["u8_" + name] = x, frame_ref(x)
    # 512 x 512: inputs regenerated from video_ref's hash, outputs kept as digests (the full arrays are ~5 MB)
    for name, d in video_ref.big_depth_cases().items():
        rgba, out["vmm_" + name] = depth_ref(d)
        out["sha_rgba_" + name] = np.array(video_ref.digest(rgba))
    for name, x in video_ref.big_image_cases().items():
        out["sha_u8_" + name] = np.array(video_ref.digest(frame_ref(x)))
    cm = matplotlib.colormaps["jet"]
    cm._init()
    out["lut_jet"] = (cm._lut * 255).astype(np.uint8)
    path = os.path.join(HERE, "ref_video_fixtures.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
