"""Bits of the passes behind a finished forward (median depth / ids, depth distortion, and their backwards), as SHA-256 digests:
for a change that must leave them alone.  Run it on both builds; the two outputs must be equal.

    python tools/side_pass_digest.py [--out FILE]

Inputs: the box inputs of tests/distort_ref.py INPUTS (tests/median_ref.py's sparse, dense, small; wide; thin) and its posed case --
ragged image edges, pixels without a median, lists longer than one staging round, footprints on both sides of the median
backward's limits.  Every input under default and strict parity, forward shapes fwd_pair 0 and 2, the activated and the raw entry
point and both distortion maps, in exact mode, through the binding's own calls (_C.rasterize_gaussians[_raw], render_median,
median_backward, render_distortion, distortion_backward).  One case hashes, in this order: median depth, median ids, the median's
dL/dmeans3D under a seeded upstream, distortion, moments, and the six gradients of the distortion under a seeded upstream (None:
nothing).  Prints ONE JSON line {case: digest}; needs a HIP device.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GRADS = ("means2D", "opacity", "means3D", "scales", "rotations", "cov3D")


def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def case_digest(name, raw, mapping, dev):
    from luciddreamer_amd import _C
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    from luciddreamer_amd.rasterizer import GaussianRasterizationSettings
    from tests import distort_ref as dr, helpers as hp
    cam, cloud, degree, bg = dr.case(name)
    H, W = cam.image_height, cam.image_width
    c = cam.to(dev)
    tfx, tfy = hp.tan_fov(cam)
    bg = bg.to(dev)
    rs = GaussianRasterizationSettings(H, W, tfx, tfy, bg, 1.0, c.world_view_transform, c.full_proj_transform, degree,
                                       c.camera_center, False, False)
    cl = {k: v.detach().to(dev).contiguous() for k, v in cloud.items()}
    if raw:
        pc = GaussianCloud(cl["means3D"], cl["scales"], cl["rotations"], cl["opacities"], cl["shs"], active_sh_degree=degree)
        m3, op, sc, rot = (t.detach() for t in (pc._xyz, pc._opacity, pc._scaling, pc._rotation))
        out = _C.rasterize_gaussians_raw(bg, m3, pc._features_dc.detach(), pc._features_rest.detach(), op, sc, rot, 1.0,
                                         rs.viewmatrix, rs.projmatrix, tfx, tfy, H, W, degree, rs.campos, False)
    else:
        m3, op, sc, rot = cl["means3D"], cl["opacities"], cl["scales"], cl["rotations"]
        out = _C.rasterize_gaussians(bg, m3, None, op, sc, rot, 1.0, None, rs.viewmatrix, rs.projmatrix, tfx, tfy, H, W,
                                     cl["shs"], degree, rs.campos, False, False)
    radii, geom, binning, img = out[3], out[4], out[5], out[6]
    P = m3.shape[0]
    depth, ids = _C.render_median(geom, binning, img, P, H, W)
    g_med = _C.median_backward(geom, binning, img, radii, ids, dr.upstream(H, W, seed=41).to(dev), rs.viewmatrix)
    dist, mom = _C.render_distortion(geom, binning, img, P, H, W, distortion_map=mapping)
    g = _C.distortion_backward(geom, binning, img, dr.upstream(H, W).to(dev), dist, mom, rs, means3D=m3, opacities=op, scales=sc,
                               rotations=rot, raw=raw, distortion_map=mapping)
    return _digest([depth, ids, g_med, dist, mom] + [g[k] for k in GRADS])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib, config
    from tests import distort_ref as dr
    print(_lib.lib().lr_version().decode(), file=sys.stderr)          # which build this is; the JSON holds digests only
    config.set_async(False)
    out = {}
    try:
        for name in sorted(dr.INPUTS) + ["posed"]:
            for strict in (False, True):
                config.set_strict_parity(strict)
                for shape in (0, 2):
                    _lib.tune_set("fwd_pair", shape)
                    for raw in (False, True):
                        for mapping in sorted(dr.MAPS):
                            key = f"{name}/{'strict' if strict else 'default'}/fwd_pair{shape}/{'raw' if raw else 'activated'}/{mapping}"
                            out[key] = case_digest(name, raw, mapping, dev)
    finally:
        _lib.tune_set("fwd_pair", -1)
        config.set_strict_parity(False)
        config.set_async(True)
    text = json.dumps(out, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
