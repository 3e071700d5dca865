"""GPU: every gradient row of the rasterizer held to its OWN scale (tests/rowbar.py) on the cases of tests/rowbar_cases.py.

Each test runs the HIP path, the float64 reference and the float32 calibrators on the same inputs and applies row_bar to every
gradient tensor the mode produces: err <= max(GRAD_RTOL * row_max, 4 * e32[row]) per row, a zero reference row exactly zero,
an all-zero row where the reference is not fails, at most 2 rows per tensor excused and only if they touch a pixel the C oracle
flags as sitting on a discrete threshold.  tests/test_rowbar_cpu.py shows on the CPU what the tensor-wide bar of
helpers.compare_grads lets through and that the references alone pass this one with no row excused.

The figures in the docstrings are those printed on the MI355X: per tensor the worst err / row_max, the rows above the floor
GRAD_RTOL * row_max (they pass by the calibrators' arm or are excused) and the rows excused."""
import copy

import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, config, parallel
from tests import helpers as hp, rowbar as rb, rowbar_cases as rc
from tests import test_gpu_alpha as al

pytestmark = pytest.mark.gpu

# the backward knobs of the default build (include/lucid_raster.h, lr_tune_set), as tests/test_gpu_variants.py sets them
BACKWARD_KNOBS = [("blend_quad", 0), ("blend_quad", 1), ("blend_quad", 2), ("bwd_seg", 0), ("bwd_seg", 1), ("bwd_red", 4),
                  ("strict", 1)]
RAW_PARAMS = rc.RAW_NAMES[1:]
CAPACITY = 200_000


@pytest.fixture(autouse=True)
def _restore():
    yield
    for knob in sorted({k for k, _ in BACKWARD_KNOBS}):
        _lib.tune_set(knob, -1)
    config.set_depth_gradient(False)
    config.set_strict_parity(False)
    config.set_antialiasing(False)
    config.set_absgrad(False)


def _bg():
    return torch.tensor(rc.BG)


def _default(case, dev):
    """The public GaussianRasterizer, helpers.run_hip's way."""
    return hp.run_hip(case["cloud"], case["cam"], case["degree"], _bg(), dev, case["g_color"], colors_precomp=case["colors_precomp"],
                      cov3D_precomp=case["cov3D_precomp"], scale_modifier=case["scale_modifier"])


def _check(name, got, what, mode="color", c_oracle=None):
    """row_bar on every tensor of the case against float64 autograd in `mode`; calibrators: the same in float32 and, for the
    colour loss, the C oracle.  c_oracle: the C-oracle result whose flagged pixels may excuse a row (default: the case's own)."""
    case = rc.make(name)
    c = rc.c_oracle(name) if c_oracle is None else c_oracle
    cals = [rc.torch_grads(name, torch.float32, mode)] + ([c["grads"]] if mode == "color" else [])
    return rb.check_all(got, rc.torch_grads(name, torch.float64, mode), cals, case["names"], rb.fragile_rows_of(c), what)


# ---- the default path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.NAMES)
def test_default_path(hip_device, name):
    """Every case through the public GaussianRasterizer.  Observed on the MI355X, worst err / row_max per tensor (rows above the
    floor in brackets where there are any; no row excused anywhere):
      case               means2D   opacity      means3D   scales    rotations  sh (precomp: cov3D, colors)
      sparse_deg0        1.8e-05   4.7e-04 (2)  1.8e-05   4.6e-05   1.8e-05    1.6e-05
      sparse_deg1        1.9e-05   2.3e-04 (2)  1.9e-05   3.0e-05   3.6e-05    1.6e-05
      sparse_deg2        1.8e-05   2.0e-03 (3)  1.9e-05   2.3e-05   2.6e-05    1.6e-05
      sparse_deg3        1.8e-05   3.2e-04 (2)  1.9e-05   2.0e-05   2.7e-05    1.6e-05
      occluded           1.0e-05   6.6e-05      8.2e-06   1.0e-05   1.5e-05    4.7e-06
      posed              2.4e-05   4.7e-04 (1)  2.6e-05   6.8e-05   5.2e-05    2.1e-05
      fov_clamp          1.3e-05   3.4e-05      2.0e-05   8.7e-06   5.4e-06    2.7e-06
      sh_clamp           5.7e-05   1.5e-04 (1)  3.4e-05   2.5e-05   3.6e-05    1.5e-05
      precomp            2.8e-05   5.5e-04 (1)  1.6e-05   1.5e-05 (cov3D)      1.5e-05 (colors)
      scale_modifier     7.7e-06   6.0e-05      2.0e-05   1.1e-05   2.1e-05    1.3e-05
      long_lists         2.4e-05   2.7e-04 (1)  1.6e-05   1.5e-05   2.0e-05    5.0e-06
      constant_upstream  1.9e-05   1.3e-05      1.3e-05   4.3e-06   6.2e-06    1.2e-06
    Only dL/dopacity has rows above the floor: a sum over the pixels of terms of both signs, where the two CPU restatements
    are as far from float64 as the kernel is."""
    case = rc.make(name)
    hip = _default(case, hip_device)
    assert np.array_equal(hip["radii"] > 0, rc.c_oracle(name)["radii"] > 0)
    _check(name, hip["grads"], f"default path, {name}")


# ---- the kernel variants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob,value", BACKWARD_KNOBS, ids=[f"{k}{v}" for k, v in BACKWARD_KNOBS])
@pytest.mark.parametrize("name", ["occluded", "sparse_deg3", "long_lists"])
def test_backward_variants(hip_device, name, knob, value):
    """The tile kernels (k_render_bwd_tile, _tile7, _tile_swap, the QUAD form), whole lists instead of segments, the checked
    candidate loop and the strict blend: until now compared with each other and with the tensor-wide bar only.  No list of
    `occluded` or `sparse_deg3` is longer than one segment (173 and 70 entries): bwd_seg changes the walk on `long_lists` only
    (three of its four lists hold 268 to 291).
    Observed: under the six knobs other than strict the figures of test_default_path or close to them (dL/dopacity: occluded
    6.4e-05 to 8.9e-05, sparse_deg3 3.2e-04 with 2 rows above the floor, long_lists 2.7e-04 with 1); strict = 1 moves
    dL/dopacity (occluded 2.0e-04 with 1 row above the floor, sparse_deg3 3.2e-04 with 3, long_lists 4.0e-04 with 1).  The other
    tensors stay at or below 3.0e-05 with no row above the floor; no row excused."""
    _lib.tune_set(knob, value)
    hip = _default(rc.make(name), hip_device)
    _check(name, hip["grads"], f"{knob} = {value}, {name}")


# ---- the raw path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse_deg3", "occluded"])
def test_raw_path(hip_device, name):
    """render_raw on stored parameters (logit opacity, log scale, quaternions with norms from 0.5 to 2): the RAW lines of
    gauss_backward_one -- the exp, the quaternion projection, the sigmoid factor -- against the float64 oracle with the
    activations written in torch in front of it; calibrator: the same chain in float32.
    Observed (means2D, _xyz, _opacity, _scaling, _rotation, _features_dc, _features_rest): sparse_deg3 1.7e-05, 2.2e-05,
    3.1e-04 (2 rows above the floor), 2.9e-05, 2.5e-05, 1.6e-05, 1.6e-05; occluded 1.5e-05, 9.0e-06, 1.2e-04 (1 row), 6.4e-06,
    1.2e-05, 4.4e-06, 4.6e-06; no row excused."""
    from luciddreamer_amd.gaussian_renderer import render_raw
    case = rc.make(name)
    stored, _ = rc.raw_cloud(name)
    model = copy.copy(stored)
    for n in RAW_PARAMS:
        setattr(model, n, getattr(stored, n).detach().to(hip_device).requires_grad_(True))
    out = render_raw(case["cam"].to(hip_device), model, bg_color=_bg().to(hip_device))
    (out["render"] * case["g_color"].to(hip_device)).sum().backward()
    got = {n: getattr(model, n).grad.detach().cpu().numpy() for n in RAW_PARAMS}
    got["means2D"] = out["viewspace_points"].grad.detach().cpu().numpy()
    norms = stored._rotation.detach().norm(dim=1)
    assert float(norms.min()) < 0.6 and float(norms.max()) > 1.8
    rb.check_all(got, rc.raw_torch_grads(name), [rc.raw_torch_grads(name, torch.float32)], rc.RAW_NAMES,
                 rb.fragile_rows_of(rc.raw_c_oracle(name)), f"raw path, {name}")


# ---- depth and alpha modes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["depth", "alpha", "all"])
@pytest.mark.parametrize("name", ["occluded", "posed"])
def test_depth_and_alpha_modes(hip_device, name, mode):
    """Upstream gradients on depth only, on alpha only, and on colour + depth + alpha: k_render_bwd_depth, _alpha, _depth_alpha
    and k_gauss_bwd_depth (the V[2], V[6], V[10] depth term under the posed camera) against tests/grad_oracle.render in float64,
    calibrated by the same in float32.
    Observed (means2D, opacity, means3D, scales, rotations, sh; rows above the floor in brackets, none excused):
      occluded  depth  1.9e-05  1.5e-04 (1)  1.5e-05  1.2e-05  2.3e-05      0
                alpha  1.6e-05  1.1e-04 (1)  9.2e-06  5.1e-05  3.1e-05      0
                all    2.7e-05  1.2e-04 (1)  8.9e-06  1.5e-05  1.9e-05      4.7e-06
      posed     depth  9.3e-05  1.2e-04 (2)  3.4e-05  2.8e-05  1.4e-04 (1)  0
                alpha  2.8e-05  1.6e-04 (2)  2.5e-05  2.5e-05  6.9e-05      0
                all    3.9e-05  2.7e-04 (3)  3.4e-05  3.7e-05  3.2e-05      2.1e-05
    dL/dsh of a loss on depth or alpha alone is exactly zero, as in the reference."""
    case = rc.make(name)
    gc = case["g_color"] if mode == "all" else None
    gd = rc.upstream_depth(case) if mode in ("depth", "all") else None
    ga = rc.upstream_alpha(case) if mode in ("alpha", "all") else None
    config.set_depth_gradient(gd is not None)
    hip = al._run(case["cloud"], case["cam"], case["degree"], _bg(), hip_device, gc, gd, ga, return_alpha=ga is not None)
    got = _check(name, hip["grads"], f"{mode} loss, {name}", mode=mode)
    if mode != "all":
        assert got["sh"]["worst"] == 0.0 and float(np.abs(hip["grads"]["sh"]).max()) == 0.0       # colours get nothing
    assert float(np.abs(hip["grads"]["means3D"]).max()) > 0.0


# ---- anti-aliasing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse_deg3", "occluded"])
def test_antialiased(hip_device, name):
    """opacity * coef with the coefficient's own derivative (tests/aa_ref.py's chain in float64; calibrator: in float32, the
    cancellation of det0 included).
    Observed (means2D, opacity, means3D, scales, rotations, sh): sparse_deg3 1.6e-05, 5.1e-04 (1 row above the floor), 1.7e-05,
    2.8e-05, 2.2e-05, 1.6e-05; occluded 1.7e-05, 2.6e-05, 1.2e-05, 6.9e-06, 3.1e-05, 4.7e-06; no row excused."""
    from tests import aa_cases
    case = rc.make(name)
    cam, cloud = case["cam"], case["cloud"]
    c = hp.run_oracle(aa_cases.prescaled(cloud, aa_cases.coef_of(cam, cloud)), cam, case["degree"], _bg(), case["g_color"])
    config.set_antialiasing(True)
    hip = _default(case, hip_device)
    _check(name, hip["grads"], f"antialiased, {name}", mode="aa", c_oracle=c)
    plain = rc.torch_grads(name)["scales"]
    assert np.abs(rc.torch_grads(name, torch.float64, "aa")["scales"] - plain).max() > 1e-2 * np.abs(plain).max()


# ---- AbsGS --------------------------------------------------------------------------------------------------------------------
def test_absgrad_rows(hip_device):
    """dL_dmean2D_abs of `occluded` against the float64 sum over the pixels of the magnitudes of every pixel's share
    (rowbar_cases.abs_reference: tests/absgrad_ref.py's quantity).  All-positive sums: float32 stays at the floor.
    Observed: worst err / row_max 2.5e-06 over the 300 rows (the float32 restatement: 2.2e-06), no row above the floor, none
    excused; the signed dL/dmeans2D of the same call 1.3e-05."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    name = "occluded"
    case = rc.make(name)
    cam, cloud = case["cam"].to(hip_device), case["cloud"]
    tfx, tfy = hp.tan_fov(case["cam"])
    d = lambda t: t.detach().to(hip_device).requires_grad_(True)
    m3 = d(cloud["means3D"])
    m2 = torch.zeros_like(m3, requires_grad=True)
    rs = GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=tfx, tanfovy=tfy, bg=_bg().to(hip_device),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=case["degree"],
        campos=cam.camera_center, prefiltered=False, debug=False)
    config.set_absgrad(True)
    config.set_async(False)
    try:
        out = GaussianRasterizer(rs)(means3D=m3, means2D=m2, opacities=d(cloud["opacities"]), shs=d(cloud["shs"]),
                                     scales=d(cloud["scales"]), rotations=d(cloud["rotations"]))
        (out[0] * case["g_color"].to(hip_device)).sum().backward()
    finally:
        config.set_async(True)
    a = m2.absgrad.detach().cpu().numpy()
    assert a.shape == (m3.shape[0], 3) and (a[:, 2] == 0).all() and (a >= 0).all()
    ref, _ = rc.abs_reference(name)
    cal, _ = rc.abs_reference(name, torch.float32)
    rep = rb.check_all({"abs": a[:, :2]}, {"abs": ref}, [{"abs": cal}], ["abs"], rb.fragile_rows_of(rc.c_oracle(name)), "absgrad, occluded")
    signed = m2.grad.detach().cpu().numpy()
    rb.check_all({"means2D": signed}, rc.torch_grads(name), [rc.torch_grads(name, torch.float32), rc.c_oracle(name)["grads"]],
                 ["means2D"], rb.fragile_rows_of(rc.c_oracle(name)), "absgrad, occluded, the signed output of the same call")
    assert rep["abs"]["rows"] == 300


# ---- the multi-view step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [1, 2])
def test_multi_view_step(hip_device, n_streams):
    """Three views of `occluded` -- the identity camera and two posed ones -- through parallel.ViewBatch (lr_views_accumulate: the
    acc16 rows and k_uninterleave_add) against the float64 sum of the three views' gradients; calibrators: the float32 sum and
    the C oracle's.  A third of the rows (104 of 300) is visible in the first view only.
    Observed (means2D, opacity, means3D, scales, rotations, sh): one chain 1.1e-05, 5.6e-04 (2 rows above the floor), 9.7e-06,
    1.0e-05, 1.9e-05, 7.9e-06; two chains 1.0e-05, 3.9e-04 (3 rows), 8.9e-06, 1.0e-05, 2.0e-05, 7.1e-06; no row excused."""
    name = rc.VIEW_CASE
    case = rc.make(name)
    n = len(rc.VIEW_POSES)
    cams = [rc.view_camera(case, v).to(hip_device) for v in range(n)]
    gs = [rc.view_upstream(case, v).to(hip_device) for v in range(n)]
    cloud = {k: v.to(hip_device) for k, v in case["cloud"].items()}
    P = cloud["means3D"].shape[0]
    shapes = {"means3D": (P, 3), "means2D": (P, 3), "opacity": (P, 1), "sh": (P, 16, 3), "scales": (P, 3), "rotations": (P, 4)}
    acc = {k: torch.zeros(s, device=hip_device) for k, s in shapes.items()}
    batch = parallel.ViewBatch(cams, gs, case["degree"], _bg().to(hip_device), binning_capacity=CAPACITY, n_streams=n_streams)
    with torch.no_grad():
        batch.run(cloud["means3D"], cloud["opacities"], cloud["scales"], cloud["rotations"], cloud["shs"], acc)
    batch.check()
    per_view = [rc.c_oracle(name, None, v) for v in range(n)]
    vis = np.stack([c["radii"] > 0 for c in per_view])
    assert int((vis.sum(axis=0) == 1).sum()) >= 50
    fragile = frozenset().union(*[rb.fragile_rows_of(c) for c in per_view])
    rb.check_all({k: v.cpu().numpy() for k, v in acc.items()}, rc.view_sum(name), [rc.view_sum(name, torch.float32), rc.view_sum_c(name)],
                 case["names"], fragile, f"three views in one step, {n_streams} chain(s)")
