"""Bits of the passes behind a finished forward (median depth / ids, depth distortion, rendered normals, fused geometry, feature
map, and their backwards), as SHA-256 digests: for a change that must leave them alone.  Run it on both builds; the two outputs must
be equal.

    python tools/side_pass_digest.py [--out FILE]

Inputs: the box inputs of tests/distort_ref.py INPUTS (tests/median_ref.py's sparse, dense, small; wide; thin) and its posed case --
ragged image edges, pixels without a median, lists longer than one staging round, footprints on both sides of the median
backward's limits.  Every input under default and strict parity, forward shapes fwd_pair 0 and 2, the activated and the raw entry
point and both distortion maps, in exact mode, through the binding's own calls (_C.rasterize_gaussians[_raw], render_median,
median_backward, render_distortion, distortion_backward).  One case hashes, in this order: median depth, median ids, the median's
dL/dmeans3D under a seeded upstream, distortion, moments, and the six gradients of the distortion under a seeded upstream (None:
nothing).

The side backwards' shared host path (keys "side/..."; default parity and forward shape): per input, activated and raw,
    normals      render_normals + render_normals_backward;
    geometry     render_geometry + geometry_backward with an image upstream of both maps, a scalar distortion upstream, the
                 normals' upstream alone, and no upstream;
    featuresC    render_features + render_features_backward at C = 1, 16 (a full chunk), 19 (full + tail);
    precomp      on `sparse`: distortion_backward and render_features_backward with cov3D_precomp;
each backward twice: into new tensors, and ("+acc") with every accumulate_into target pre-filled from a seeded tensor.
    operator     on `sparse`: rasterize_gaussians[_raw] with return_median, return_distortion, return_normals and features, fused
                 gradient accumulation off and on, forward + backward twice (the second lands in the existing .grad): every leaf's
                 .grad.
    views        on `sparse`: one ViewBatch step of 3 views with distortion_weight and normal_consistency_weight: the accumulators.
Prints ONE JSON line {case: digest}; needs a HIP device.
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


def _forward(name, raw, dev, cov=None):
    """(rs, inputs of the side passes, (radii, geom, binning, img), num_rendered) of an exact-mode forward of the input `name`."""
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
        inputs = dict(means3D=m3, opacities=op, scales=sc, rotations=rot, raw=True)
    elif cov is not None:
        out = _C.rasterize_gaussians(bg, cl["means3D"], None, cl["opacities"], None, None, 1.0, cov, rs.viewmatrix, rs.projmatrix, tfx,
                                     tfy, H, W, cl["shs"], degree, rs.campos, False, False)
        inputs = dict(means3D=cl["means3D"], opacities=cl["opacities"], cov3D_precomp=cov)
    else:
        out = _C.rasterize_gaussians(bg, cl["means3D"], None, cl["opacities"], cl["scales"], cl["rotations"], 1.0, None, rs.viewmatrix,
                                     rs.projmatrix, tfx, tfy, H, W, cl["shs"], degree, rs.campos, False, False)
        inputs = dict(means3D=cl["means3D"], opacities=cl["opacities"], scales=cl["scales"], rotations=cl["rotations"])
    return rs, inputs, (out[3], out[4], out[5], out[6]), int(out[0])


def _seeded(shape, seed, dev):
    """A seeded tensor in [-1, 1): an upstream gradient, or what an accumulate_into target holds before the call."""
    return (2.0 * torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) - 1.0).to(dev)


def _twice(backward, shapes, dev):
    """{"": digest of backward(None), "+acc": digest of backward(targets pre-filled from seeded tensors)}; shapes: {name: shape}."""
    names = sorted(shapes)
    g = backward(None)
    acc = {k: _seeded(shapes[k], 100 + i, dev) for i, k in enumerate(names)}
    h = backward(acc)
    extra = sorted(k for k in g if k not in shapes)                   # gauss_normal: always a new tensor
    assert all(h[k] is acc[k] for k in names)
    return {"": _digest([g.get(k) for k in names + extra]), "+acc": _digest([h[k] for k in names + extra])}


def side_digests(name, raw, dev):
    """The normals, geometry and feature families of one input."""
    from luciddreamer_amd import _C
    from tests import distort_ref as dr
    rs, inputs, (radii, geom, binning, img), num_rendered = _forward(name, raw, dev)
    H, W, P = rs.image_height, rs.image_width, inputs["means3D"].shape[0]
    geo = {k: v for k, v in inputs.items() if k != "opacities"}
    five = {"means2D": (P, 3), "opacity": (P, 1), "means3D": (P, 3), "scales": (P, 3), "rotations": (P, 4)}
    key = lambda family: f"side/{name}/{'raw' if raw else 'activated'}/{family}"
    out = {}
    gN, gD = _seeded((3, H, W), 43, dev), dr.upstream(H, W).to(dev)
    nrm, gn = _C.render_normals(geom, binning, img, radii, rs, **geo)
    out[key("normals/forward")] = _digest([nrm, gn])
    for tag, d in _twice(lambda acc: _C.render_normals_backward(geom, binning, img, gN, nrm, gn, radii, rs, accumulate_into=acc, **inputs),
                         five, dev).items():
        out[key("normals/backward" + tag)] = d
    dist, mom, nrm2, gn2 = _C.render_geometry(geom, binning, img, radii, rs, **geo)
    out[key("geometry/forward")] = _digest([dist, mom, nrm2, gn2])
    for what, (uD, uN) in (("images", (gD, gN)), ("scalar", (0.37, None)), ("normals_only", (None, gN)), ("none", (None, None))):
        for tag, d in _twice(lambda acc: _C.geometry_backward(geom, binning, img, uD, dist, mom, uN, nrm2, gn2, radii, rs,
                                                              accumulate_into=acc, **inputs), five, dev).items():
            out[key(f"geometry/backward_{what}" + tag)] = d
    for C in (1, 16, 19):
        f = _seeded((P, C), 50 + C, dev)
        val = _C.render_features(geom, binning, img, f, rs)
        out[key(f"features{C}/forward")] = _digest([val])
        gF = _seeded((C, H, W), 60 + C, dev)
        shapes = dict(five, features=(P, C))
        for tag, d in _twice(lambda acc: _C.render_features_backward(geom, binning, img, gF, val, f, radii, rs, slots=num_rendered,
                                                                     accumulate_into=acc, **inputs), shapes, dev).items():
            out[key(f"features{C}/backward" + tag)] = d
    return out


def precomp_digests(dev):
    """distortion_backward and render_features_backward with cov3D_precomp, on `sparse`."""
    from luciddreamer_amd import _C
    from tests import aa_ref, distort_ref as dr
    _, cloud, _, _ = dr.case("sparse")
    cov = aa_ref.cov3d64(cloud["scales"].double(), cloud["rotations"].double()).float().to(dev).contiguous()
    rs, inputs, (radii, geom, binning, img), num_rendered = _forward("sparse", False, dev, cov=cov)
    H, W, P = rs.image_height, rs.image_width, cov.shape[0]
    shapes = {"means2D": (P, 3), "opacity": (P, 1), "means3D": (P, 3), "cov3D": (P, 6)}
    out = {}
    dist, mom = _C.render_distortion(geom, binning, img, P, H, W)
    gD = dr.upstream(H, W).to(dev)
    for tag, d in _twice(lambda acc: _C.distortion_backward(geom, binning, img, gD, dist, mom, rs, accumulate_into=acc, **inputs),
                         shapes, dev).items():
        out["side/sparse/precomp/distortion/backward" + tag] = d
    f, gF = _seeded((P, 19), 69, dev), _seeded((19, H, W), 79, dev)
    val = _C.render_features(geom, binning, img, f, rs)
    for tag, d in _twice(lambda acc: _C.render_features_backward(geom, binning, img, gF, val, f, radii, rs, slots=num_rendered,
                                                                 accumulate_into=acc, **inputs), dict(shapes, features=(P, 19)), dev).items():
        out["side/sparse/precomp/features19/backward" + tag] = d
    return out


def operator_digest(raw, fused, dev):
    """Every leaf's .grad after two forward + backward rounds of the operator on `sparse` with all four side outputs on."""
    from luciddreamer_amd import config, rasterizer
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    from tests import distort_ref as dr
    config.set_fused_grad_accumulation(fused)
    rs, _, _, _ = _forward("sparse", False, dev)
    _, cloud, degree, _ = dr.case("sparse")
    cl = {k: v.detach().to(dev).contiguous() for k, v in cloud.items()}
    H, W, P = rs.image_height, rs.image_width, cl["means3D"].shape[0]
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    means2D, features = torch.zeros(P, 3, device=dev, requires_grad=True), leaf(_seeded((P, 19), 69, dev))
    if raw:
        pc = GaussianCloud(cl["means3D"], cl["scales"], cl["rotations"], cl["opacities"], cl["shs"], active_sh_degree=degree)
        leaves = [leaf(t) for t in (pc._xyz, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation)]
        run = lambda: rasterizer.rasterize_gaussians_raw(leaves[0], means2D, *leaves[1:], rs, return_median=True, return_distortion=True,
                                                         return_normals=True, features=features)
    else:
        leaves = [leaf(cl[k]) for k in ("means3D", "shs", "opacities", "scales", "rotations")]
        run = lambda: rasterizer.rasterize_gaussians(leaves[0], means2D, leaves[1], None, leaves[2], leaves[3], leaves[4], None, rs,
                                                     return_median=True, return_distortion=True, return_normals=True, features=features)
    for _ in range(2):
        color, _, depth, median, _, normals, fmap, distortion = run()
        loss = sum((t * _seeded(tuple(t.shape), 80 + i, dev)).sum() for i, t in enumerate((color, depth, median, normals, fmap, distortion)))
        loss.backward()
    torch.cuda.synchronize()
    return _digest([t.grad for t in leaves + [means2D, features]])


def views_digest(dev):
    """The accumulators after one ViewBatch step of three views of `sparse` with both geometry terms."""
    from luciddreamer_amd import parallel
    from tests import distort_ref as dr
    _, inputs, _, num_rendered = _forward("sparse", False, dev)
    cam, cloud, degree, bg = dr.case("sparse")
    cl = {k: v.detach().to(dev).contiguous() for k, v in cloud.items()}
    H, W, P = cam.image_height, cam.image_width, cl["means3D"].shape[0]
    cams = [cam.to(dev)] * 3
    targets = [_seeded((3, H, W), 90 + i, dev).abs() for i in range(3)]
    acc = {"means3D": torch.zeros(P, 3, device=dev), "means2D": torch.zeros(P, 3, device=dev), "opacity": torch.zeros(P, 1, device=dev),
           "sh": torch.zeros_like(cl["shs"]), "scales": torch.zeros(P, 3, device=dev), "rotations": torch.zeros(P, 4, device=dev)}
    batch = parallel.ViewBatch(cams, None, degree, bg.to(dev), 2 * num_rendered + 1024, n_streams=3, targets=targets,
                               distortion_weight=100.0, distortion_map="ndc", normal_consistency_weight=0.05)
    batch.run(cl["means3D"], cl["opacities"], cl["scales"], cl["rotations"], cl["shs"], acc)
    batch.check()
    return _digest([acc[k] for k in sorted(acc)])


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
    fused_was = config.fused_grad_accumulation()
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
        _lib.tune_set("fwd_pair", -1)
        config.set_strict_parity(False)
        for name in sorted(dr.INPUTS) + ["posed"]:
            for raw in (False, True):
                out.update(side_digests(name, raw, dev))
        out.update(precomp_digests(dev))
        for raw in (False, True):
            for fused in (False, True):
                out[f"side/operator/{'raw' if raw else 'activated'}/{'fused' if fused else 'unfused'}"] = operator_digest(raw, fused, dev)
        out["side/views"] = views_digest(dev)
    finally:
        _lib.tune_set("fwd_pair", -1)
        config.set_strict_parity(False)
        config.set_fused_grad_accumulation(fused_was)
        config.set_async(True)
    text = json.dumps(out, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
