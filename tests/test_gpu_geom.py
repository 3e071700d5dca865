"""The fused geometry pass on the GPU, through the C ABI (lr_render_geometry, lr_geometry_backward): depth distortion and rendered
normal map in one tile walk each way.

The forward against the two float64 references (tests/distort_ref.py, tests/render_normals_ref.py) at those suites' bars and with
their fragile-pixel rules; the gradients of both upstreams together, and of each alone with the other NULL, against the sum of the
two float64 autograd gradients at GRAD_RTOL; the scalar form of dL/dD; repeatability; anti-aliasing; raw mode; the edges.  Every
test fails without the feature: the entry points do not exist there."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, config
from tests import distort_ref as dr, helpers as hp, render_normals_ref as rn

pytestmark = pytest.mark.gpu

GEO = ["means3D", "means2D", "opacity", "scales", "rotations"]
FWD_BAR = 4.0                           # x distort_ref.FWD_ERR / render_normals_ref.FWD_ERR (their comments)
GRAD_MAP = "linear"                     # the mapping whose distortion gradient has the size of the normal map's


@pytest.fixture
def exact_mode():
    config.set_async(False)
    yield
    config.set_async(True)
    config.reset()


def _settings(cam, bg, degree, dev):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings
    tfx, tfy = hp.tan_fov(cam)
    c = cam.to(dev)
    return GaussianRasterizationSettings(cam.image_height, cam.image_width, tfx, tfy, bg.to(dev), 1.0, c.world_view_transform,
                                         c.full_proj_transform, degree, c.camera_center, False, False)


def _forward(cloud, cam, dev, capacity=0):
    """(num_rendered, color, depth, radii, geom, binning, img) of the activated C-ABI forward."""
    from luciddreamer_amd import _C
    tfx, tfy = hp.tan_fov(cam)
    camd = cam.to(dev)
    return _C.rasterize_gaussians(torch.zeros(3, device=dev), cloud["means3D"].to(dev), torch.Tensor([]),
                                  cloud["opacities"].to(dev), cloud["scales"].to(dev), cloud["rotations"].to(dev), 1.0,
                                  torch.Tensor([]), camd.world_view_transform, camd.full_proj_transform, tfx, tfy,
                                  cam.image_height, cam.image_width, cloud["shs"].to(dev), 3, camd.camera_center, False, False,
                                  binning_capacity=capacity)


def _inputs(cloud, dev):
    return dict(means3D=cloud["means3D"].to(dev), scales=cloud["scales"].to(dev), rotations=cloud["rotations"].to(dev))


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("mapping", sorted(dr.MAPS))
@pytest.mark.parametrize("name", ["sparse", "dense", "wide", "thin", "posed"])
def test_forward_parity_with_the_float64_references(hip_device, exact_mode, name, mapping, strict):
    """distortion within 4 x distort_ref.FWD_ERR and normals within 4 x render_normals_ref.FWD_ERR of float64 on the pixels
    neither suite calls fragile for its own map; D >= 0, exact zeros below two layers / without a layer.  How many words differ
    from the separate passes' outputs is printed, not asserted (the expressions and their order are the same)."""
    from luciddreamer_amd import _C
    cam, cloud, degree, bg = dr.case(name)
    H, W, P = cam.image_height, cam.image_width, cloud["means3D"].shape[0]
    d, r = dr.reference(name, mapping), rn.reference(name)
    assert d["fragile"].sum() <= dr.FRAGILE_CAP * d["fragile"].size and r["fragile"].sum() <= rn.FRAGILE_CAP * r["fragile"].size
    dev = hip_device
    rs = _settings(cam, bg, degree, dev)
    config.set_strict_parity(strict)
    try:
        f = _forward(cloud, cam, dev)
        dist, mom, nrm, gn = _C.render_geometry(f[4], f[5], f[6], f[3], rs, distortion_map=mapping, **_inputs(cloud, dev))
        dist1, mom1 = _C.render_distortion(f[4], f[5], f[6], P, H, W, distortion_map=mapping)
        nrm1, gn1 = _C.render_normals(f[4], f[5], f[6], f[3], rs, **_inputs(cloud, dev))
    finally:
        config.set_strict_parity(False)
    print(name, mapping, "strict" if strict else "default", "words that differ from the separate passes: distortion %d, moments %d, "
          "normals %d, gauss_normals %d" % tuple(int((_bits(a) != _bits(b)).sum()) for a, b in
                                                 ((dist, dist1), (mom, mom1), (nrm, nrm1), (gn, gn1))))
    assert dist.shape == (1, H, W) and mom.shape == (H, W, 4) and nrm.shape == (3, H, W) and gn.shape == (P, 4)
    D, N = dist.cpu().numpy()[0], nrm.cpu().numpy()
    ok_d, ok_n = ~d["fragile"], ~r["fragile"]
    err_d = float(np.abs(D.astype(np.float64) - d["D64"])[ok_d].max())
    err_n = float(np.abs(N.astype(np.float64) - r["N64"])[:, ok_n].max())
    bar_d, bar_n = FWD_BAR * dr.FWD_ERR[(name, mapping)], FWD_BAR * rn.FWD_ERR[name]
    print(name, mapping, "distortion err %.3e bar %.3e" % (err_d, bar_d), "normals err %.3e bar %.3e" % (err_n, bar_n))
    assert err_d <= bar_d and err_n <= bar_n
    assert (D >= 0).all()
    assert not D[ok_d & (d["layers64"] < 2)].any() and D[ok_d & (d["layers64"] >= 2)].any()
    assert not N[:, ok_n & (r["layers64"] == 0)].any() and N[:, ok_n & (r["layers64"] > 0)].any()
    # the moments are what the backward needs: A is the accumulated opacity of the blended layers
    A = mom.cpu().numpy()[..., 0]
    assert (A[ok_d & (d["layers64"] == 0)] == 0).all() and (A[ok_d & (d["layers64"] > 0)] > 0).all() and (A < 1.0 + 1e-6).all()


# ---- 2. gradients -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grad_reference(name, mapping=GRAD_MAP, aa=False):
    """(G_D, G_N, float64 leaf gradients of <G_D, D>, of <G_N, N>): the two suites' shared references where they call the same
    pixels fragile (their upstreams are then zero on the same pixels); otherwise both upstreams are zeroed on the union and the
    float64 gradients are formed here, once."""
    d = dr.aa_reference(name, mapping) if aa else dr.reference(name, mapping)
    r = rn.aa_reference(name) if aa else rn.reference(name)
    if np.array_equal(d["fragile"], r["fragile"]):
        return d["G"], r["G"], d["leaf"], r["leaf"]
    assert not aa, "the anti-aliased references share one walk"
    cam, cloud, degree, bg = dr.case(name)
    H, W = cam.image_height, cam.image_width
    fragile = d["fragile"] | r["fragile"]
    Gd, Gn = dr.upstream(H, W, fragile), rn.upstream(H, W, fragile)
    leaf_d = dr.grads64(cloud, cam, degree, bg, dr.coefficients(mapping), Gd.numpy())[0]
    leaf_n = rn.grads64(cloud, cam, degree, bg, Gn.numpy())[0]
    return Gd, Gn, leaf_d, leaf_n


def _backward(f, maps, rs, cloud, dev, Gd, Gn, mapping=GRAD_MAP, **kw):
    from luciddreamer_amd import _C
    dist, mom, nrm, gn = maps
    up = lambda g: g.to(dev) if isinstance(g, torch.Tensor) else g
    return _C.geometry_backward(f[4], f[5], f[6], up(Gd), dist, mom, up(Gn), nrm, gn, f[3], rs, distortion_map=mapping,
                                **_inputs(cloud, dev), **kw)


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("name", ["sparse", "dense", "wide", "posed"])
def test_gradients_against_the_sum_of_the_float64_gradients(hip_device, exact_mode, name, strict):
    """Both upstreams: every geometric gradient within GRAD_RTOL of dr.grads64 + rn.grads64.  Each upstream alone, the other
    NULL: that suite's gradients.  Two runs: the same bits.  The colour floats of the slots carry dL/dn: dL_dgauss_normal is the
    normal suite's own intermediate, and it is exact zeros without dL_dnormals."""
    from luciddreamer_amd import _C
    cam, cloud, degree, bg = dr.case(name)
    Gd, Gn, leaf_d, leaf_n = _grad_reference(name)
    both = {k: leaf_d[k] + leaf_n[k] for k in GEO}
    dev = hip_device
    rs = _settings(cam, bg, degree, dev)
    config.set_strict_parity(strict)
    try:
        f = _forward(cloud, cam, dev)
        maps = _C.render_geometry(f[4], f[5], f[6], f[3], rs, distortion_map=GRAD_MAP, **_inputs(cloud, dev))
        got = _backward(f, maps, rs, cloud, dev, Gd, Gn)
        again = _backward(f, maps, rs, cloud, dev, Gd, Gn)
        only_d = _backward(f, maps, rs, cloud, dev, Gd, None)
        only_n = _backward(f, maps, rs, cloud, dev, None, Gn)
        none = _backward(f, maps, rs, cloud, dev, None, None)
    finally:
        config.set_strict_parity(False)
    for label, out, want in (("both", got, both), ("distortion alone", only_d, leaf_d), ("normals alone", only_n, leaf_n)):
        o = _np(out)
        for k in GEO:
            ref = want[k]
            print(name, label, k, "err %.2e of max |g| = %.3e" % (np.abs(o[k].reshape(ref.shape) - ref).max() / np.abs(ref).max(),
                                                                 np.abs(ref).max()))
        hp.compare_grads(o, want, names=GEO)
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k
        assert not none[k].any(), k
    for k in ("means3D", "opacity", "scales"):                        # the share of each term in the sum
        print(name, k, "max |g|: distortion %.3e, normals %.3e" % (np.abs(leaf_d[k]).max(), np.abs(leaf_n[k]).max()))
    r = rn.reference(name)
    if Gn is r["G"]:
        hp.compare_grads(dict(n=got["gauss_normal"].cpu().numpy()), dict(n=r["mid"]["n"]), names=["n"])
    assert torch.equal(got["gauss_normal"], only_n["gauss_normal"])                      # dL/dn does not depend on the distortion
    assert not only_d["gauss_normal"].any()
    assert not only_d["rotations"][f[3] <= 0].any()


def test_scalar_upstream_is_the_constant_image(hip_device, exact_mode):
    """dL_ddistortion NULL with a scalar: the bits of the image filled with that scalar (the step's weight / (H W)); accumulate
    mode adds what write mode writes."""
    from luciddreamer_amd import _C
    cam, cloud, degree, bg = dr.case("sparse")
    H, W = cam.image_height, cam.image_width
    dev = hip_device
    rs = _settings(cam, bg, degree, dev)
    _, Gn, _, _ = _grad_reference("sparse")
    f = _forward(cloud, cam, dev)
    maps = _C.render_geometry(f[4], f[5], f[6], f[3], rs, distortion_map=GRAD_MAP, **_inputs(cloud, dev))
    c = 0.37 / (H * W)
    image = _backward(f, maps, rs, cloud, dev, torch.full((1, H, W), float(np.float32(c)), dtype=torch.float32), Gn)
    scalar = _backward(f, maps, rs, cloud, dev, float(np.float32(c)), Gn)
    assert image["means3D"].any()
    for k in image:
        assert np.array_equal(_bits(image[k]), _bits(scalar[k])), k
    acc = {k: torch.full_like(v, 2.0) for k, v in image.items() if k != "gauss_normal"}
    added = _backward(f, maps, rs, cloud, dev, float(np.float32(c)), Gn, accumulate_into=acc)
    vis = (f[3] > 0)
    for k, t in acc.items():
        assert added[k] is t
        touched = (t != 2.0).reshape(t.shape[0], -1).any(dim=1)
        assert not touched[~vis].any(), k                                                   # rows without an instance stay
        assert float((t - 2.0 - image[k]).abs().max()) <= 4e-7 * max(1.0, float(image[k].abs().max()) + 2.0), k


def test_gradients_with_antialiasing_on(hip_device, exact_mode):
    """The blend sees opacity x coef: both float64 references under anti-aliasing, both upstreams."""
    from luciddreamer_amd import _C
    name = "sparse"
    cam, cloud, degree, bg = dr.case(name)
    Gd, Gn, leaf_d, leaf_n = _grad_reference(name, GRAD_MAP, True)
    d, r = dr.aa_reference(name, GRAD_MAP), rn.aa_reference(name)
    dev = hip_device
    rs = _settings(cam, bg, degree, dev)
    config.set_antialiasing(True)
    try:
        f = _forward(cloud, cam, dev)
        maps = _C.render_geometry(f[4], f[5], f[6], f[3], rs, distortion_map=GRAD_MAP, **_inputs(cloud, dev))
        got = _np(_C.geometry_backward(f[4], f[5], f[6], Gd.to(dev), maps[0], maps[1], Gn.to(dev), maps[2], maps[3], f[3], rs,
                                       distortion_map=GRAD_MAP, opacities=cloud["opacities"].to(dev), **_inputs(cloud, dev)))
    finally:
        config.set_antialiasing(False)
    ok = ~d["fragile"]
    assert np.abs(maps[0].cpu().numpy()[0].astype(np.float64) - d["D64"])[ok].max() <= FWD_BAR * dr.FWD_ERR[(name, GRAD_MAP)]
    assert np.abs(maps[2].cpu().numpy().astype(np.float64) - r["N64"])[:, ~r["fragile"]].max() <= FWD_BAR * rn.FWD_ERR[name]
    hp.compare_grads(got, {k: leaf_d[k] + leaf_n[k] for k in GEO}, names=GEO)


def test_raw_mode_gradients(hip_device, exact_mode):
    """The stored parameters on "posed": log-scales, logit-opacities, quaternions before normalisation."""
    from luciddreamer_amd import _C
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    name = "posed"
    cam, cloud, degree, bg = dr.case(name)
    Gd, Gn, leaf_d, leaf_n = _grad_reference(name)
    want = dr.raw_grads(cloud, {k: leaf_d[k] + leaf_n[k] for k in GEO})
    dev = hip_device
    rs = _settings(cam, bg, degree, dev)
    pc = GaussianCloud(cloud["means3D"].to(dev), cloud["scales"].to(dev), cloud["rotations"].to(dev), cloud["opacities"].to(dev),
                       cloud["shs"].to(dev), active_sh_degree=degree)
    tfx, tfy = hp.tan_fov(cam)
    camd = cam.to(dev)
    f = _C.rasterize_gaussians_raw(bg.to(dev), pc._xyz, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation,
                                   1.0, camd.world_view_transform, camd.full_proj_transform, tfx, tfy, cam.image_height,
                                   cam.image_width, degree, camd.camera_center, False)
    stored = dict(means3D=pc._xyz.detach(), scales=pc._scaling.detach(), rotations=pc._rotation.detach(), raw=True)
    maps = _C.render_geometry(f[4], f[5], f[6], f[3], rs, distortion_map=GRAD_MAP, **stored)
    r = rn.reference(name)
    assert np.abs(maps[2].cpu().numpy().astype(np.float64) - r["N64"])[:, ~r["fragile"]].max() <= FWD_BAR * rn.FWD_ERR[name]
    out = _np(_C.geometry_backward(f[4], f[5], f[6], Gd.to(dev), maps[0], maps[1], Gn.to(dev), maps[2], maps[3], f[3], rs,
                                   distortion_map=GRAD_MAP, opacities=pc._opacity.detach(), **stored))
    got = dict(xyz=out["means3D"], means2D=out["means2D"], opacity=out["opacity"], scaling=out["scales"], rotation=out["rotations"])
    for k in want:
        print(name, "raw", k, "err %.2e" % (np.abs(got[k].reshape(want[k].shape) - want[k]).max() / np.abs(want[k]).max()))
    hp.compare_grads(got, want, names=list(want))


# ---- 3. edges -----------------------------------------------------------------------------------------------------------------
def test_c_abi_edges(hip_device):
    from luciddreamer_amd import _C
    cam, cloud, degree, bg = dr.case("sparse")
    H, W, P = cam.image_height, cam.image_width, cloud["means3D"].shape[0]
    dev = hip_device
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rs = _settings(cam, bg, degree, dev)
    inputs = _inputs(cloud, dev)
    exact = _forward(cloud, cam, dev)
    m0 = _C.render_geometry(exact[4], exact[5], exact[6], exact[3], rs, **inputs)
    assert m0[0].any() and m0[2].any()
    # a capacity that holds the view: the exact forward's outputs
    cap = 4 * int(exact[0]) + 1024
    roomy = _forward(cloud, cam, dev, cap)
    m1 = _C.render_geometry(roomy[4], roomy[5], roomy[6], roomy[3], rs, binning_capacity=cap, **inputs)
    assert all(torch.equal(a, b) for a, b in zip(m0, m1))
    # an async forward whose binning capacity is too small: zeros, rc 0, the overflow is lr_check's to report; nothing is added
    over = _forward(cloud, cam, dev, 100)
    m = _C.render_geometry(over[4], over[5], over[6], over[3], rs, binning_capacity=100, **inputs)
    assert not m[0].any() and not m[1].any() and not m[2].any()
    with pytest.raises(RuntimeError, match="capacity"):
        _C.check(over[4])
    Gd, Gn = torch.ones(1, H, W, device=dev), torch.ones(3, H, W, device=dev)
    acc = {k: torch.full(s, 3.0, device=dev) for k, s in (("means2D", (P, 3)), ("opacity", (P, 1)), ("means3D", (P, 3)),
                                                            ("scales", (P, 3)), ("rotations", (P, 4)))}
    o = _C.geometry_backward(over[4], over[5], over[6], Gd, m[0], m[1], Gn, m[2], m[3], over[3], rs, binning_capacity=100,
                             accumulate_into=acc, **inputs)
    assert all(bool((t == 3.0).all()) for t in acc.values()) and not o["gauss_normal"].any()
    o = _C.geometry_backward(over[4], over[5], over[6], Gd, m[0], m[1], Gn, m[2], m[3], over[3], rs, binning_capacity=100, **inputs)
    assert all(not t.any() for t in o.values())
    # P = 0: zeros, no buffer read (none is given); the backward has nothing to do
    d0, q0, n0 = torch.ones(1, H, W, device=dev), torch.ones(H, W, 4, device=dev), torch.ones(3, H, W, device=dev)
    a = _lib.GeometryArgs(view=_lib.View(P=0, width=W, height=H), out_distortion=d0.data_ptr(), out_moments=q0.data_ptr(),
                          out_normals=n0.data_ptr(), stream=stream)
    assert L.lr_render_geometry(a) == 0
    assert L.lr_geometry_backward(_lib.GeometryBackwardArgs(view=_lib.View(P=0, width=W, height=H), stream=stream)) == 0
    torch.cuda.synchronize()
    assert not d0.any() and not q0.any() and not n0.any()
    # cov3D_precomp has no normal: refused by both entries and by the wrappers, before any launch
    with pytest.raises(ValueError, match="cov3D_precomp"):
        _C.render_geometry(exact[4], exact[5], exact[6], exact[3], rs, means3D=inputs["means3D"], scales=None, rotations=None,
                           cov3D_precomp=torch.zeros(P, 6, device=dev))
    cov = torch.zeros(P, 6, device=dev)
    state = dict(geom_buffer=exact[4].data_ptr(), binning_buffer=exact[5].data_ptr(), image_buffer=exact[6].data_ptr())
    v = _lib.View(P=P, width=W, height=H, means3D=inputs["means3D"].data_ptr(), cov3D_precomp=cov.data_ptr())
    a = _lib.GeometryArgs(view=v, radii=exact[3].data_ptr(), out_distortion=d0.data_ptr(), out_moments=q0.data_ptr(),
                          out_normals=n0.data_ptr(), out_gauss_normals=m0[3].data_ptr(), stream=stream, **state)
    assert L.lr_render_geometry(a) == _lib.LR_ERR_INVALID_ARG and b"cov3D_precomp" in L.lr_last_error()
    b = _lib.GeometryBackwardArgs(view=v, stream=stream, **state)
    assert L.lr_geometry_backward(b) == _lib.LR_ERR_INVALID_ARG and b"cov3D_precomp" in L.lr_last_error()
    # a wrong struct_bytes, with everything else in place
    a.view.cov3D_precomp = None
    a.struct_bytes = ctypes.sizeof(_lib.GeometryArgs) - 8
    assert L.lr_render_geometry(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    b.struct_bytes = ctypes.sizeof(_lib.GeometryBackwardArgs) + 8
    assert L.lr_geometry_backward(b) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    torch.cuda.synchronize()
    assert not d0.any()                                                                     # the refused calls wrote nothing
