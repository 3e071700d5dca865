"""The two geometry regularisers inside the multi-view step on the GPU (ViewBatch(distortion_weight=, normal_consistency_weight=)
-> lr_views_accumulate -> lr_render_geometry / lr_geometry_backward per view).

The yardstick is the per-view route: render(..., return_distortion=True, return_normals=True), l1_dssim + w_d D.mean() +
rendered_normal_consistency(N, depth), one autograd backward per view, summed -- a route that is itself held to float64 in its
own suites (tests/test_gpu_distort.py, tests/test_gpu_render_normals.py, tests/test_gpu_normals.py).  Every accumulator must lie
within GRAD_RTOL of its tensor's largest entry; every loss column is compared with the per-view values at the bar of the term's
own suite.  Then: weight 0, absent arguments, chains, repeatability, the map outputs, the densification statistics.  Every test
fails without the feature: ViewBatch does not take the arguments there."""
import numpy as np
import pytest
import torch

from luciddreamer_amd import config, synthetic
from tests import helpers as hp, posed_cases as pc_

pytestmark = pytest.mark.gpu

KEYS = {"means3D": "means3D", "means2D": "means2D", "opacity": "opacities", "sh": "shs", "scales": "scales", "rotations": "rotations"}
# three cameras around the box cloud's own (identity) camera: the cloud stays in view of each
POSES = ((0.0, 0.0, 0.0, (0.0, 0.0, 0.0)), (0.05, -0.03, 0.1, (0.15, -0.1, 0.1)), (-0.06, 0.04, -0.2, (-0.2, 0.1, -0.3)))
# name: P, W, H, scale_mult, seed -- the sizes of distort_ref's "sparse", of posed_cases' box cases, and of "wide" (lists over many tiles)
SCENES = {"sparse": (2000, 70, 45, 1.0, 0), "posed": (1500, 70, 45, 1.5, 2), "wide": (1000, 150, 110, 4.0, 0)}
W_D, W_N, MAPPING = 0.8, 0.3, "linear"
CAPACITY = 400_000


@pytest.fixture
def depth_on():
    """The per-view route differentiates the depth output (the normal term's dL/ddepth)."""
    config.set_depth_gradient(True)
    yield
    config.set_depth_gradient(False)


def _scene(name, dev):
    P, W, H, s, seed = SCENES[name]
    cloud = {k: v.to(dev) for k, v in synthetic.make_cloud(P, "box", seed, scale_mult=s).items()}
    cams = [pc_.camera(p, W, H).to(dev) for p in POSES]
    gen = torch.Generator().manual_seed(11)
    targets = [torch.rand(3, H, W, generator=gen).to(dev) for _ in cams]
    return cloud, cams, targets


def _raster(c, bg, degree=3):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    tfx, tfy = hp.tan_fov(c)
    return GaussianRasterizer(GaussianRasterizationSettings(c.image_height, c.image_width, tfx, tfy, bg, 1.0, c.world_view_transform,
                                                            c.full_proj_transform, degree, c.camera_center, False, False))


def _acc(cloud):
    P, dev = cloud["means3D"].shape[0], cloud["means3D"].device
    return {"means3D": torch.zeros_like(cloud["means3D"]), "means2D": torch.zeros(P, 3, device=dev),
            "opacity": torch.zeros_like(cloud["opacities"]), "sh": torch.zeros_like(cloud["shs"]),
            "scales": torch.zeros_like(cloud["scales"]), "rotations": torch.zeros_like(cloud["rotations"])}


def _step(cloud, cams, targets, bg, n_streams=2, stats=None, **kw):
    """One ViewBatch step on zeroed accumulators: (accumulators, losses [n, columns], the batch)."""
    from luciddreamer_amd import parallel
    batch = parallel.ViewBatch(cams, None, 3, bg, binning_capacity=CAPACITY, n_streams=n_streams, targets=targets, lambda_dssim=0.2,
                               **kw)
    acc = _acc(cloud)
    with torch.no_grad():
        batch.run(cloud["means3D"], cloud["opacities"], cloud["scales"], cloud["rotations"], cloud["shs"], acc, stats=stats)
    batch.check()
    return acc, batch.losses.clone(), batch


def _consistency64(N, depth, cam):
    """(float64 value of sum_valid (1 - N.n) / (H W) on the device's own N and depth, e_n): the restatement and the bar's e_n of
    tests/test_gpu_render_normals.py::test_rendered_normal_consistency_against_its_float64_restatement."""
    from tests import normal_ref as nr, rowbar
    tx, ty = hp.tan_fov(cam)
    H, W = depth.shape[-2:]
    d = depth.detach().cpu().numpy().reshape(H, W)
    n64, valid = nr.torch_normals(torch.from_numpy(d).double(), tx, ty)
    want = torch.where(valid, 1.0 - (N.detach().cpu().double() * n64).sum(0), torch.zeros(H, W, dtype=torch.float64)).sum() / (H * W)
    n32, _ = nr.closed_normals(d, tx, ty, np.float32)
    e_n = max(rowbar.E32_MARGIN * float(np.abs(n32 - n64.numpy()).max()), 16 * 2.0 ** -24)
    return float(want), e_n, int(valid.sum())


def _per_view(cloud, cams, targets, bg, w_d, w_n, mapping=MAPPING, depth_targets=None, depth_weight=0.0, masks=None, alpha_weight=0.0):
    """The parent's route: one autograd pass per view, gradients summed.  Returns (gradients, per-view rows of
    {loss, l1-dssim part, depth term, alpha hole, mean D, consistency}, the maps, the float64 consistency values and bars)."""
    from luciddreamer_amd import normals
    from luciddreamer_amd.loss import alpha_hole, depth_l1, l1_dssim_loss, masked_l1_dssim
    P = cloud["means3D"].shape[0]
    leaf = {k: v.clone().requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros(P, 3, device=cloud["means3D"].device, requires_grad=True)
    rows, maps, c64 = [], [], []
    config.set_async(False)
    try:
        for i, (c, tgt) in enumerate(zip(cams, targets)):
            out = _raster(c, bg)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"], shs=leaf["shs"],
                                 scales=leaf["scales"], rotations=leaf["rotations"], return_alpha=masks is not None,
                                 return_normals=True, return_distortion=True, distortion_map=mapping)
            col, dep, N, D = out[0], out[2], out[-2], out[-1]
            lc = l1_dssim_loss(col, tgt, 0.2) if masks is None else masked_l1_dssim(col, tgt, masks[i], 0.2)
            ld = depth_l1(dep, depth_targets[i]) if depth_targets is not None else torch.zeros((), device=col.device)
            la = alpha_hole(out[3], masks[i]) if masks is not None else torch.zeros((), device=col.device)
            md = D.mean()
            cn = normals.rendered_normal_consistency(N, dep, c, weight=1.0)
            loss = lc + depth_weight * ld + alpha_weight * la + w_d * md + w_n * cn
            loss.backward()
            rows.append([float(x.detach()) for x in (loss, lc, ld, la, md, cn)])
            maps.append((D.detach().clone(), N.detach().clone(), dep.detach().clone()))
            c64.append(_consistency64(N, dep, c))
    finally:
        config.set_async(True)
        config.reset()
    ref = {k: v.grad.clone() for k, v in leaf.items()}
    ref["means2D"] = m2d.grad.clone()
    return ref, np.array(rows, np.float64), maps, c64


def _compare_acc(acc, ref, label):
    got = {k: acc[k].cpu().numpy() for k in KEYS}
    want = {k: ref[rk].cpu().numpy() for k, rk in KEYS.items()}
    for k in KEYS:
        scale = np.abs(want[k]).max()
        print(label, k, "err %.2e of max |g| = %.3e" % (np.abs(got[k].reshape(want[k].shape) - want[k]).max() / scale, scale))
    hp.compare_grads(got, want, names=list(KEYS))


def _compare_losses(losses, rows, maps, c64, w_d, w_n, label, min_valid=0.2):
    """Columns {loss, l1, ssim, depth term, alpha_hole, distortion, normal_consistency} against the per-view values.  min_valid: the
    share of the pixels that must have a normal from depth (the scene's fitness, not a bar)."""
    got = losses.cpu().numpy().astype(np.float64)
    assert got.shape == (len(rows), 7)
    H, W = maps[0][0].shape[-2:]
    for v in range(len(rows)):
        loss, lc, ld, la, md, cn = rows[v]
        # the colour part, the depth term and the alpha hole term: the bars of their step suites (1e-5 of the value)
        assert abs((0.8 * got[v, 1] + 0.2 * (1.0 - got[v, 2])) - lc) <= 1e-5 * abs(lc), (label, v)
        assert abs(got[v, 3] - ld) <= 1e-5 * abs(ld) and abs(got[v, 4] - la) <= 1e-5 * abs(la), (label, v, got[v], ld, la)
        # mean(D): the step's map is the per-view map (asserted where the maps are returned), its mean is formed in double and
        # rounded once.  The per-view float32 mean of n = H W <= 16 500 terms >= 0 is a tree sum over partial sums of a few terms
        # each: at most log2(n) + 8 < 24 roundings on any term's way to the total, one more for the division -- 32 x 2^-24 of it
        d64 = float(maps[v][0].double().mean())
        assert abs(got[v, 5] - d64) <= 2.0 ** -22 * d64 and d64 > 0, (label, v, got[v, 5], d64)
        assert abs(got[v, 5] - md) <= 32 * 2.0 ** -24 * d64, (label, v, got[v, 5], md)
        # the consistency value: both sides within the e_n-based bar of the float64 restatement on the view's own N and depth
        want64, e_n, n_valid = c64[v]
        bar = 3 * e_n + 2.0 ** -20
        print(label, "view", v, "consistency %.6f, float64 %.6f, per view %.6f, bar %.2e, valid pixels %d of %d" %
              (got[v, 6], want64, cn, bar, n_valid, H * W))
        assert n_valid > min_valid * H * W, (label, v, n_valid)
        assert abs(got[v, 6] - want64) <= bar and abs(cn - want64) <= bar, (label, v, got[v, 6], cn, want64, bar)
        assert abs(got[v, 0] - loss) <= 1e-5 * abs(loss) + w_n * 2 * bar, (label, v, got[v, 0], loss)


# ---- 1. against the per-view route --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_streams", [("sparse", 1), ("sparse", 2), ("posed", 1), ("posed", 2), ("wide", 2)])
def test_both_terms_equal_the_per_view_route(hip_device, depth_on, name, n_streams):
    """3 views; with n_streams = 2 the first slot is reused within the step.  150 x 110 runs once."""
    cloud, cams, targets = _scene(name, hip_device)
    bg = torch.tensor([0.1, 0.0, 0.2], device=hip_device)
    ref, rows, maps, c64 = _per_view(cloud, cams, targets, bg, W_D, W_N)
    acc, losses, _ = _step(cloud, cams, targets, bg, n_streams, distortion_weight=W_D, distortion_map=MAPPING,
                           normal_consistency_weight=W_N)
    label = "%s n_streams=%d" % (name, n_streams)
    _compare_acc(acc, ref, label)
    _compare_losses(losses, rows, maps, c64, W_D, W_N, label)
    assert not losses[:, 3].any() and not losses[:, 4].any()                              # absent terms are 0
    # the terms are in: the colour-only step differs
    plain, _, _ = _step(cloud, cams, targets, bg, n_streams)
    for k in ("means3D", "scales", "rotations"):
        assert float((plain[k] - acc[k]).abs().max()) > 100 * hp.GRAD_RTOL * float(acc[k].abs().max()), k


@pytest.mark.parametrize("which", ["distortion", "normals"])
def test_each_term_alone_equals_the_per_view_route(hip_device, depth_on, which):
    cloud, cams, targets = _scene("sparse", hip_device)
    bg = torch.tensor([0.0, 0.1, 0.0], device=hip_device)
    w_d, w_n = (W_D, 0.0) if which == "distortion" else (0.0, W_N)
    mapping = "ndc" if which == "distortion" else MAPPING
    ref, rows, maps, c64 = _per_view(cloud, cams, targets, bg, w_d, w_n, mapping)
    kw = dict(distortion_weight=W_D) if which == "distortion" else dict(normal_consistency_weight=W_N)
    kw["distortion_map"] = mapping                                                        # (also what the reported mean(D) is of)
    acc, losses, _ = _step(cloud, cams, targets, bg, 2, **kw)
    _compare_acc(acc, ref, which + " alone")
    _compare_losses(losses, rows, maps, c64, w_d, w_n, which + " alone")                  # the other term is still reported


def test_both_terms_with_depth_targets_and_masks(hip_device, depth_on):
    from luciddreamer_amd.loss import content_mask
    name = "posed"
    cloud, cams, targets = _scene(name, hip_device)
    _, W, H, _, _ = SCENES[name]
    bg = torch.zeros(3, device=hip_device)
    gen = torch.Generator().manual_seed(5)
    holed, masks, dts = [], [], []
    for t in targets:
        hole = (torch.rand(1, H, W, generator=gen) < 0.2).to(hip_device)
        holed.append(torch.where(hole, torch.zeros_like(t), t).contiguous())
        masks.append(content_mask(holed[-1]))
        dt = 2.0 + 6.0 * torch.rand(1, H, W, generator=gen)
        dts.append(torch.where(torch.rand(1, H, W, generator=gen) < 0.3, torch.zeros_like(dt), dt).to(hip_device))
    dw, aw = 0.35, 0.6
    ref, rows, maps, c64 = _per_view(cloud, cams, holed, bg, W_D, W_N, depth_targets=dts, depth_weight=dw, masks=masks, alpha_weight=aw)
    acc, losses, _ = _step(cloud, cams, holed, bg, 2, distortion_weight=W_D, distortion_map=MAPPING, normal_consistency_weight=W_N,
                           depth_targets=dts, depth_weight=dw, masks=masks, alpha_weight=aw)
    _compare_acc(acc, ref, "all terms")
    _compare_losses(losses, rows, maps, c64, W_D, W_N, "all terms")
    assert bool((losses[:, 3] > 0).all()) and bool((losses[:, 4] > 0).all())


# ---- 2. weights of 0, absent arguments ------------------------------------------------------------------------------------------
def test_weights_of_zero_report_the_terms_and_absent_arguments_are_todays_step(hip_device):
    cloud, cams, targets = _scene("sparse", hip_device)
    bg = torch.tensor([0.1, 0.0, 0.2], device=hip_device)
    plain, plain_losses, b0 = _step(cloud, cams, targets, bg, 2)
    zero, zero_losses, b1 = _step(cloud, cams, targets, bg, 2, distortion_weight=0.0, distortion_map=MAPPING,
                                  normal_consistency_weight=0.0)
    on, on_losses, _ = _step(cloud, cams, targets, bg, 2, distortion_weight=W_D, distortion_map=MAPPING, normal_consistency_weight=W_N)
    assert tuple(plain_losses.shape) == (3, 3) and tuple(zero_losses.shape) == (3, 7)
    for k in plain:
        assert torch.equal(plain[k], zero[k]), k                                        # the bits of the step without the arguments
    assert torch.equal(zero_losses[:, :3], plain_losses)
    assert torch.equal(zero_losses[:, 5:], on_losses[:, 5:]) and bool((zero_losses[:, 5:] > 0).all())   # reported all the same
    assert not zero_losses[:, 3:5].any()
    # one weight 0: the gradients of the step with the other term alone, to the bit
    only_d, ld, _ = _step(cloud, cams, targets, bg, 2, distortion_weight=W_D, distortion_map=MAPPING)
    d_and_0, l0, _ = _step(cloud, cams, targets, bg, 2, distortion_weight=W_D, distortion_map=MAPPING, normal_consistency_weight=0.0)
    for k in only_d:
        assert torch.equal(only_d[k], d_and_0[k]), k
    assert torch.equal(ld, l0)
    # today's step, to the bit, also next to a batch with the terms: the workspace of one is not the other's
    again, again_losses, _ = _step(cloud, cams, targets, bg, 2)
    for k in plain:
        assert torch.equal(plain[k], again[k]), k
    assert torch.equal(plain_losses, again_losses)
    assert b1.workspace.numel() > b0.workspace.numel()


# ---- 3. determinism, the maps --------------------------------------------------------------------------------------------------
def test_same_bits_for_every_number_of_chains_and_the_maps_are_the_pass_outputs(hip_device):
    from luciddreamer_amd import _C
    name = "posed"
    cloud, cams, targets = _scene(name, hip_device)
    P, W, H, _, _ = SCENES[name]
    bg = torch.tensor([0.1, 0.0, 0.2], device=hip_device)
    want = want_losses = want_maps = None
    for n_streams in (1, 2, 2, 3):
        dists = [torch.full((1, H, W), -1.0, device=hip_device) for _ in cams]
        nmaps = [torch.full((3, H, W), -1.0, device=hip_device) for _ in cams]
        acc, losses, _ = _step(cloud, cams, targets, bg, n_streams, distortion_weight=W_D, distortion_map=MAPPING,
                               normal_consistency_weight=W_N, distortions=dists, normal_maps=nmaps)
        if want is None:
            want, want_losses, want_maps = acc, losses, (dists, nmaps)
            assert all(float(v.abs().sum()) > 0 for v in want.values())
            continue
        for k in want:
            assert torch.equal(acc[k], want[k]), (n_streams, k)
        assert torch.equal(losses, want_losses), n_streams
        for a, b in zip(dists + nmaps, want_maps[0] + want_maps[1]):
            assert torch.equal(a, b), n_streams
    # the maps are what lr_render_geometry writes behind the same forward
    config.set_async(False)
    try:
        for c, D, N in zip(cams, *want_maps):
            tfx, tfy = hp.tan_fov(c)
            f = _C.rasterize_gaussians(bg, cloud["means3D"], torch.Tensor([]), cloud["opacities"], cloud["scales"], cloud["rotations"],
                                       1.0, torch.Tensor([]), c.world_view_transform, c.full_proj_transform, tfx, tfy, H, W,
                                       cloud["shs"], 3, c.camera_center, False, False, binning_capacity=0)
            rs = _raster(c, bg).raster_settings
            d1, _, n1, _ = _C.render_geometry(f[4], f[5], f[6], f[3], rs, distortion_map=MAPPING, means3D=cloud["means3D"],
                                              scales=cloud["scales"], rotations=cloud["rotations"])
            assert torch.equal(D, d1) and torch.equal(N, n1) and bool(D.any()) and bool(N.any())
    finally:
        config.set_async(True)
        config.reset()


# ---- 4. the densification statistics --------------------------------------------------------------------------------------------
def test_statistics_keep_meaning_the_photometric_gradient(hip_device):
    """densify_stats="grad" with the terms on: the geometry pass passes no stat_accum, so with the distortion term on (and the
    normal term reported) the three tensors have the bits of the step without the arguments, while the gradients do carry the
    term.  A normal weight > 0 puts that term's dL/ddepth into the view's depth-gradient image, which the view's blend backward
    -- and with it the gradient statistic -- sees as part of the view's depth gradient (include/lucid_raster.h says so): the
    visit half (denom, max_radii2D) stays exact, and asking for the statistics leaves the step's gradients bit for bit."""
    cloud, cams, targets = _scene("sparse", hip_device)
    P = cloud["means3D"].shape[0]
    bg = torch.tensor([0.1, 0.0, 0.2], device=hip_device)
    new = lambda: {"xyz_gradient_accum": torch.zeros(P, 1, device=hip_device), "denom": torch.zeros(P, 1, device=hip_device),
                   "max_radii2D": torch.zeros(P, device=hip_device)}
    s0, s1, s2 = new(), new(), new()
    plain, _, _ = _step(cloud, cams, targets, bg, 2, stats=s0, densify_stats="grad")
    dist, _, _ = _step(cloud, cams, targets, bg, 2, stats=s1, densify_stats="grad", distortion_weight=W_D, distortion_map=MAPPING,
                       normal_consistency_weight=0.0)
    assert bool(s0["xyz_gradient_accum"].any()) and bool(s0["denom"].any())
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert float((dist["means2D"] - plain["means2D"]).abs().max()) > 0                   # while the gradients do have the term
    both, _, _ = _step(cloud, cams, targets, bg, 2, stats=s2, densify_stats="grad", distortion_weight=W_D, distortion_map=MAPPING,
                       normal_consistency_weight=W_N)
    assert torch.equal(s0["denom"], s2["denom"]) and torch.equal(s0["max_radii2D"], s2["max_radii2D"])
    no_stats, _, _ = _step(cloud, cams, targets, bg, 2, distortion_weight=W_D, distortion_map=MAPPING, normal_consistency_weight=W_N)
    for k in both:
        assert torch.equal(both[k], no_stats[k]), k                                      # "grad" leaves the step's gradients bit for bit
    assert bool(torch.isfinite(s2["xyz_gradient_accum"]).all())
