#!/usr/bin/env python
"""A LucidDreamer-style optimisation loop (/root/reference/luciddreamer.py:221-327) on synthetic data, using every
piece of this repository on the MI355X:

    render_raw        rasterizer fed with the stored parameters (activations inside the kernels)      8a-8d, 8f-2
    l1_dssim_loss     fused (1-l)*L1 + l*(1-SSIM) and its gradient                                     8f-3
    densify           densify_and_prune / prune through one row-selection kernel, Adam state intact     8f-4
    FusedAdam         torch.optim.Adam's arithmetic in one launch per step                              (8e: the step after the all-reduce)
    distCUDA2         initial scales from the 3-nearest-neighbour distance                              8f-1
    MCMCStrategy      --mcmc: relocation, capped growth and position noise instead of densify_and_prune   DESIGN.md 4b-MCMC
    filter3d          --filter3d: the 3D smoothing filter of Mip-Splatting on what the rasterizer is shown   DESIGN.md 4b-F3D
    normals           --normal-weight / --normal-consistency: normals from depth and the fused normal losses  DESIGN.md 4b-NRM

Targets are renders of a hidden "ground truth" cloud from a look-around camera path; the trained cloud starts from
a perturbed subset of it.  Prints the loss every `--log` iterations and the time per iteration.

    python examples/train_loop.py [--gaussians 200000] [--iters 300] [--resolution 512x512]
                                  [--absgrad --densify-grad-threshold 0.0008]
                                  [--multi-view 4 [--absgrad]]
                                  [--mcmc --cap-max 150000]
                                  [--multi-view 4 --depth-weight 0.1 [--depth-loss pearson]]
                                  [--filter3d [--antialiasing]]
                                  [--normal-weight 0.05] [--normal-consistency 0.05] [--distortion-weight 100]
                                  [--rendered-normal-consistency 0.05]
                                  [--feature-channels 16]

--multi-view K: the loop body is ONE multi-view step (parallel.ViewBatch: forward, L1 + DSSIM loss and backward of K views in one
C call, gradients summed) followed by Adam; the densification statistics are formed inside the step, per view
(densify_stats="grad", or "absgrad" with --absgrad), and densify_and_prune runs on them.

--multi-view K --depth-weight W: the step also supervises every view's rendered depth with the hidden cloud's depth map
(ViewBatch(depth_targets=, depth_weight=W)).  --depth-loss l1 compares absolute values (loss.depth_l1); --depth-loss pearson
compares by correlation (loss.depth_pearson), and the example then CORRUPTS every view's depth target by a per-view random scale
a in [0.5, 2] and shift b in [-1, 1] -- what a monocular estimate does to it -- which that term does not see and an L1 term
would be pulled apart by.

--mcmc --cap-max N: in either loop the MCMC strategy (luciddreamer_amd.mcmc.MCMCStrategy) takes the place of the densify_and_prune
calls: the regularisers' gradients are added before the optimizer's step, and after it dead Gaussians are relocated and the set
grows by 5 % -- never beyond N -- on the --densify-from / --densify-every / --densify-until schedule, with the position noise
every iteration.  No gradient threshold and no densification statistics are involved.

--normal-weight W (single-view loop): the rendered depth's normals are held to the normals of the hidden cloud's depth map
(normals.depth_normals of it, no gradient: what a monocular normal estimate would be) by normals.normal_loss with weight W, with
the depth gradient on (config.set_depth_gradient).  --normal-consistency W: the forward also returns the median depth
(return_median=True) and normals.normal_consistency(depth, median_depth) with weight W is added; the median's side of it moves
the means only.  The multi-view step has no normal term of its own: a caller reaches it through ViewBatch(grad_depths=).

--distortion-weight W: the forward also returns the depth distortion (return_distortion=True: Mip-NeRF 360's
distortion loss as 2DGS uses it, on the "ndc" mapping) and W x its mean over the image is added to the loss.

--rendered-normal-consistency W: the forward also returns the rendered normal map (return_normals=True: the
blend of the Gaussians' own normals, their shortest axes turned towards the camera) and
normals.rendered_normal_consistency(normals, depth) with weight W is added: the normal consistency of 2DGS / RaDe-GS / PGSR,
which turns the Gaussians' flat sides into the surface the rendered depth describes.  Turns the depth gradient on.
With --multi-view K both terms run inside the step (ViewBatch(distortion_weight=W, normal_consistency_weight=W)): one fused pass
each way per view behind the blend forward and the colour backward, the same loss as the single-view loop's.

--depth-smoothness W (single-view loop): smooth.depth_smoothness of the rendered depth, guided by the target image, with weight W
is added: the edge-aware smoothness term of the Monodepth lineage / DNGaussian / MonoGS, which keeps the depth smooth where the
image is and lets it jump at image edges.  --smoothness-order 1 or 2 (first or second differences), --smoothness-space depth
or inverse (on 1 / depth).  Turns the depth gradient on.

--feature-channels C (single-view loop): a [P,C] feature table is rendered next to the colour (render_raw(features=table):
lr_render_features, 16 channels per tile walk) and trained in a torch Adam group of its own with L1 against a fixed seeded [C,3]
projection of the target image; the term is printed with the loss.  The set of Gaussians stays fixed: a table has no
densification surgery.

--filter3d: in either loop the rasterizer is shown the cloud through luciddreamer_amd.filter3d.filtered(model, filter): every
Gaussian low-passed by the highest sampling rate at which a training camera sees it (the 3D smoothing filter of Mip-Splatting).
The filter is computed after build, again after every densify / prune / MCMC change of the set (a filter of another length than
the model raises), and every 100 iterations once densification has stopped.  The single-view loop renders the stored-domain view
through render_raw, the multi-view loop feeds the view's activated getters to ViewBatch.run.  Independent of --antialiasing (the
2D Mip filter): either works without the other, Mip-Splatting uses both.
"""
import argparse
import math
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from luciddreamer_amd import cameras, config, densify, filter3d, mcmc, synthetic     # noqa: E402
from luciddreamer_amd.gaussian_renderer import GaussianCloud, render_raw   # noqa: E402
from luciddreamer_amd.loss import l1_dssim_loss                            # noqa: E402
from luciddreamer_amd.normals import depth_normals, normal_consistency, normal_loss, rendered_normal_consistency     # noqa: E402
from luciddreamer_amd.smooth import depth_smoothness                       # noqa: E402
from luciddreamer_amd.optim import FusedAdam                               # noqa: E402
from simple_knn._C import distCUDA2                                        # noqa: E402

GROUP_ATTR = densify.GROUP_ATTR


class TrainableCloud(GaussianCloud):
    """GaussianCloud + what GaussianModel.training_setup adds (scene/gaussian_model.py:148-169)."""

    def training_setup(self, lrs, percent_dense=0.01, torch_adam=False):
        P = self._xyz.shape[0]
        dev = self._xyz.device
        for a in GROUP_ATTR.values():
            setattr(self, a, torch.nn.Parameter(getattr(self, a).detach().clone().requires_grad_(True)))
        self.percent_dense = percent_dense
        self.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        self.denom = torch.zeros((P, 1), device=dev)
        self.max_radii2D = torch.zeros((P,), device=dev)
        groups = [{"params": [getattr(self, a)], "lr": lrs[n], "name": n} for n, a in GROUP_ATTR.items()]
        self.optimizer = (torch.optim.Adam if torch_adam else FusedAdam)(groups, lr=0.0, eps=1e-15)

    def add_densification_stats(self, viewspace_point_tensor, update_filter):     # gaussian_model.py:405-407
        # same sums as the reference's boolean-mask indexing, written without the host synchronisation that indexing
        # with a mask implies (nonzero): rows outside the filter add 0
        f = update_filter[:, None].float()
        self.xyz_gradient_accum += f * torch.norm(viewspace_point_tensor.grad[:, :2], dim=-1, keepdim=True)
        self.denom += f


def build(args, dev):
    W, H = (int(v) for v in args.resolution.split("x"))
    gt_cloud = {k: v.to(dev) for k, v in synthetic.make_cloud(args.gaussians, "box", 0).items()}
    gt = GaussianCloud(gt_cloud["means3D"], gt_cloud["scales"], gt_cloud["rotations"], gt_cloud["opacities"], gt_cloud["shs"],
                       requires_grad=False)
    cams = [c.to(dev) for c in cameras.lookaround_path(W, H, n_views=args.views)]
    with torch.no_grad():
        targets = [render_raw(c, gt, render_only=True)["render"].clamp(0, 1) for c in cams]
    # start: every second Gaussian, jittered; scales from the 3-NN distance like create_from_pcd (gaussian_model.py:136-137)
    g = torch.Generator(device="cpu").manual_seed(1)
    idx = torch.arange(0, args.gaussians, 2, device=dev)
    xyz = gt_cloud["means3D"][idx] + 0.01 * torch.randn(idx.numel(), 3, generator=g).to(dev)
    dist2 = torch.clamp_min(distCUDA2(xyz.contiguous()), 1e-7)
    scales = torch.sqrt(dist2)[:, None].repeat(1, 3)
    rots = torch.zeros(idx.numel(), 4, device=dev)
    rots[:, 0] = 1
    shs = torch.zeros(idx.numel(), 16, 3, device=dev)
    shs[:, 0] = gt_cloud["shs"][idx, 0]
    model = TrainableCloud(xyz, scales, rots, torch.full((idx.numel(), 1), 0.1, device=dev), shs)
    model.training_setup({"xyz": LR_XYZ, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3},
                         torch_adam=args.torch_adam)
    return model, cams, targets


def depth_targets_for(args, dev):
    """--depth-weight: the hidden cloud's depth per view (0 where it covers nothing: no target there); with --depth-loss pearson
    every view's map is corrupted by its own scale a in [0.5, 2] and shift b in [-1, 1], as estimated depth is."""
    W, H = (int(v) for v in args.resolution.split("x"))
    gt_cloud = {k: v.to(dev) for k, v in synthetic.make_cloud(args.gaussians, "box", 0).items()}
    gt = GaussianCloud(gt_cloud["means3D"], gt_cloud["scales"], gt_cloud["rotations"], gt_cloud["opacities"], gt_cloud["shs"],
                       requires_grad=False)
    cams = [c.to(dev) for c in cameras.lookaround_path(W, H, n_views=args.views)]
    with torch.no_grad():
        depths = [render_raw(c, gt, render_only=True)["depth"].reshape(1, H, W).contiguous() for c in cams]
    if args.depth_loss == "pearson":
        g = torch.Generator(device="cpu").manual_seed(2)
        for i, d in enumerate(depths):
            a, b = 0.5 + 1.5 * float(torch.rand(1, generator=g)), -1.0 + 2.0 * float(torch.rand(1, generator=g))
            depths[i] = torch.where(d > 0, (a * d + b).clamp_min(1e-3), d)       # a pixel with a target keeps one
    return depths


def normal_targets_for(args, dev):
    """--normal-weight: per view, the normals of the hidden cloud's depth map ((0,0,0) where it has none: no target there)."""
    W, H = (int(v) for v in args.resolution.split("x"))
    gt_cloud = {k: v.to(dev) for k, v in synthetic.make_cloud(args.gaussians, "box", 0).items()}
    gt = GaussianCloud(gt_cloud["means3D"], gt_cloud["scales"], gt_cloud["rotations"], gt_cloud["opacities"], gt_cloud["shs"],
                       requires_grad=False)
    cams = [c.to(dev) for c in cameras.lookaround_path(W, H, n_views=args.views)]
    with torch.no_grad():
        return [depth_normals(render_raw(c, gt, render_only=True)["depth"].reshape(1, H, W).contiguous(), c) for c in cams]


LR_XYZ = 1.6e-4                # the position learning rate of build(): the noise is scaled by it


def _mcmc_strategy(args, model):
    """--mcmc: the strategy on the loop's densification schedule (--cap-max 0: 1.5 x the initial count)."""
    if not getattr(args, "mcmc", False):
        return None
    cap = int(args.cap_max) if int(args.cap_max) > 0 else int(1.5 * model._xyz.shape[0])
    return mcmc.MCMCStrategy(cap, refine_start=args.densify_from, refine_stop=args.densify_until, refine_every=args.densify_every)


class _Filter3D:
    """--filter3d: the filter of the current set of Gaussians and the view of the model under it (the model itself without)."""
    REFRESH = 100                  # iterations between two updates once densification has stopped

    def __init__(self, args, model, cams, dev):
        self.on = bool(getattr(args, "filter3d", False))
        self.filter = None
        if self.on:
            self.cams = filter3d.pack_cameras(cams, dev)
            self.update(model)

    def update(self, model):
        if self.on:
            self.filter = filter3d.compute_filter_3d(model._xyz.detach(), self.cams)

    def after_step(self, model, it, changed, densify_until):
        """The set changed (densify / prune / MCMC), or densification is over and REFRESH iterations have passed."""
        if changed or (it >= densify_until and it % self.REFRESH == 0):
            self.update(model)

    def view(self, model):
        return filter3d.filtered(model, self.filter) if self.on else model


def _capacity(model, cams, bg):
    """Binning capacity of a multi-view step: twice the largest exact-mode instance count over the path, + 4096 (the cloud
    moves between two densifications; an overflow is reported by ViewBatch.check, never silent)."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd import _C
    config.set_async(False)
    try:
        n = []
        with torch.no_grad():
            for c in cams:
                rs = GaussianRasterizationSettings(c.image_height, c.image_width, math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5),
                                                   bg, 1.0, c.world_view_transform, c.full_proj_transform, 3, c.camera_center,
                                                   False, False)
                GaussianRasterizer(rs)(means3D=model.get_xyz, means2D=torch.zeros_like(model.get_xyz), opacities=model.get_opacity,
                                       shs=model.get_features.contiguous(), scales=model.get_scaling, rotations=model.get_rotation)
                n.append(int(_C.last_num_rendered()))
    finally:
        config.set_async(True)
        config.reset()
    return 2 * max(n) + 4096


def train_multi_view(args, log=print):
    """One ViewBatch step of K views with targets per iteration, then Adam; densification on the step's own statistics."""
    from luciddreamer_amd import parallel
    dev = torch.device("cuda:0")
    model, cams, targets = build(args, dev)
    bg = torch.zeros(3, device=dev)
    K = min(int(args.multi_view), len(cams))
    mode = "absgrad" if args.absgrad else "grad"
    config.set_antialiasing(args.antialiasing)
    groups = [list(range(i, i + K)) for i in range(0, len(cams) - K + 1, K)]      # consecutive views of the path
    f3 = _Filter3D(args, model, cams, dev)
    batches, cap = {}, _capacity(f3.view(model), cams, bg)
    depth_weight = float(getattr(args, "depth_weight", 0.0))
    dts = depth_targets_for(args, dev) if depth_weight > 0 else None
    # the two geometry regularisers run inside the step: one fused pass each way per view (lr_render_geometry / lr_geometry_backward)
    distortion_w = float(getattr(args, "distortion_weight", 0.0))
    rendered_w = float(getattr(args, "rendered_normal_consistency", 0.0))
    geom = {}
    if distortion_w > 0:
        geom.update(distortion_weight=distortion_w, distortion_map="ndc")
    if rendered_w > 0:
        geom.update(normal_consistency_weight=rendered_w)

    def batch_for(gi, with_stats):
        key = (gi, with_stats)
        if key not in batches:
            depth = {} if dts is None else dict(depth_targets=[dts[i] for i in groups[gi]], depth_weight=depth_weight,
                                                depth_loss=args.depth_loss)
            depth.update(geom)
            batches[key] = parallel.ViewBatch([cams[i] for i in groups[gi]], None, 3, bg, cap, n_streams=min(3, K),
                                              targets=[targets[i] for i in groups[gi]], lambda_dssim=args.lambda_dssim,
                                              densify_stats=mode if with_stats else None, **depth)
        return batches[key]
    losses = []
    gen = torch.Generator().manual_seed(0)
    strategy = _mcmc_strategy(args, model)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(1, args.iters + 1):
        gi = int(torch.randint(0, len(groups), (1,), generator=gen))
        with_stats = strategy is None and it < args.densify_until
        batch = batch_for(gi, with_stats)
        # the step takes activated parameters and accumulates their gradients; autograd carries them to the stored ones
        shown = f3.view(model)                     # --filter3d: the activated getters of the filtered view
        act = {"means3D": model.get_xyz, "opacities": shown.get_opacity, "scales": shown.get_scaling,
               "rotations": model.get_rotation, "shs": model.get_features}
        P = act["means3D"].shape[0]
        acc = {"means3D": torch.zeros(P, 3, device=dev), "means2D": torch.zeros(P, 3, device=dev),
               "opacity": torch.zeros(P, 1, device=dev), "sh": torch.zeros(P, 16, 3, device=dev),
               "scales": torch.zeros(P, 3, device=dev), "rotations": torch.zeros(P, 4, device=dev)}
        d = {k: v.detach().contiguous() for k, v in act.items()}
        batch.run(d["means3D"], d["opacities"], d["scales"], d["rotations"], d["shs"], acc,
                  stats=densify.view_batch_stats(model) if with_stats else None)
        torch.autograd.backward([act["means3D"], act["opacities"], act["scales"], act["rotations"], act["shs"]],
                                [acc["means3D"], acc["opacity"], acc["scales"], acc["rotations"], acc["sh"]])
        with torch.no_grad():
            densified = with_stats and it >= args.densify_from and it % args.densify_every == 0
            if densified:
                batch.check()                      # an overflowed view would have contributed nothing
                densify.densify_and_prune(model, args.densify_grad_threshold, 0.005, 5.0, 20)
            if strategy is not None:
                strategy.add_regularizer_grads(model)
            model.optimizer.step()
            model.optimizer.zero_grad(set_to_none=True)
            if strategy is not None:               # relocated Gaussians sit elsewhere, added ones change P
                densified = any(strategy.step(model, it, LR_XYZ))
            f3.after_step(model, it, densified, args.densify_until)
            if densified:                          # another P: another capacity, and the batches are rebuilt on it
                batches, cap = {}, _capacity(f3.view(model), cams, bg)
        if it % args.log == 0 or it == 1:
            batch.check()
            losses.append((it, float(batch.losses[:, 0].mean().item()), int(model._xyz.shape[0])))
            log(f"iter {it:5d}  loss {losses[-1][1]:.5f}  gaussians {losses[-1][2]}")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    config.set_antialiasing(False)
    log(f"{args.iters} iterations of {K} views in {dt:.2f} s = {dt / args.iters * 1e3:.3f} ms/iteration")
    return losses, dt


def train(args, log=print):
    normal_w, consistency_w = getattr(args, "normal_weight", 0.0), getattr(args, "normal_consistency", 0.0)
    distortion_w = getattr(args, "distortion_weight", 0.0)
    rendered_w = getattr(args, "rendered_normal_consistency", 0.0)
    smooth_w = getattr(args, "depth_smoothness", 0.0)
    feature_c = int(getattr(args, "feature_channels", 0))
    if feature_c > 0 and (getattr(args, "multi_view", 0) > 0 or getattr(args, "mcmc", False)):
        raise SystemExit("--feature-channels: the single-view loop with a fixed set of Gaussians only (the multi-view step has no "
                         "feature pass, and a feature table has no densification surgery)")
    if getattr(args, "multi_view", 0) > 0:
        if normal_w > 0 or consistency_w > 0 or smooth_w > 0:
            raise SystemExit("--normal-weight / --normal-consistency / --depth-smoothness: the single-view loop only (the "
                             "multi-view step takes an external depth term through ViewBatch(grad_depths=))")
        return train_multi_view(args, log)
    dev = torch.device("cuda:0")
    model, cams, targets = build(args, dev)
    normal_targets = normal_targets_for(args, dev) if normal_w > 0 else None
    depth_terms = normal_w > 0 or consistency_w > 0 or rendered_w > 0 or smooth_w > 0
    if depth_terms:
        config.set_depth_gradient(True)            # the normal and smoothness terms act on the rendered depth
    bg = torch.zeros(3, device=dev)
    # no host round trip per forward ("Host sync"); instance counts drift while the cloud is
    # optimised, so the capacity is taken over the views of the path, with generous headroom
    config.set_async(not args.exact, headroom=1.5, warm_calls=len(cams))     # overflowed views are re-rendered (default policy)
    config.set_antialiasing(args.antialiasing)     # opacity compensation for the 2D dilation; render the result with it on too
    config.set_absgrad(args.absgrad)               # AbsGS: the backward attaches viewspace_points.absgrad, the statistics use it
    losses = []
    gen = torch.Generator().manual_seed(0)
    strategy = _mcmc_strategy(args, model)
    f3 = _Filter3D(args, model, cams, dev)
    # --feature-channels C: a [P,C] table rendered next to the colour (features=: lr_render_features), trained in a torch Adam
    # group of its own with L1 against a fixed seeded [C,3] projection of the target image.  The set of Gaussians stays as it is:
    # a table has no densification surgery.
    table = table_opt = projection = None
    if feature_c > 0:
        fgen = torch.Generator().manual_seed(1)
        table = torch.zeros(model._xyz.shape[0], feature_c, device=dev, requires_grad=True)
        table_opt = torch.optim.Adam([table], lr=0.0025, eps=1e-15)          # the rate of features_dc
        projection = (torch.randn(feature_c, 3, generator=fgen) / 3.0 ** 0.5).to(dev)
    feature_term = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(1, args.iters + 1):
        v = int(torch.randint(0, len(cams), (1,), generator=gen))
        pkg = render_raw(cams[v], f3.view(model), bg_color=bg, return_median=consistency_w > 0,    # luciddreamer.py:296
                         return_distortion=distortion_w > 0, return_normals=rendered_w > 0, features=table)
        loss = l1_dssim_loss(pkg["render"], targets[v], args.lambda_dssim)                # :301-303
        if table is not None:
            feature_term = (pkg["features"] - torch.einsum("ck,khw->chw", projection, targets[v])).abs().mean()
            loss = loss + feature_term
        if normal_w > 0:
            loss = loss + normal_loss(pkg["depth"], normal_targets[v], cams[v], weight=normal_w)
        if consistency_w > 0:
            loss = loss + normal_consistency(pkg["depth"], pkg["median_depth"], cams[v], weight=consistency_w)
        if distortion_w > 0:
            loss = loss + distortion_w * pkg["distortion"].mean()
        if rendered_w > 0:
            loss = loss + rendered_normal_consistency(pkg["normals"], pkg["depth"], cams[v], weight=rendered_w)
        if smooth_w > 0:
            loss = loss + depth_smoothness(pkg["depth"], targets[v], order=args.smoothness_order, space=args.smoothness_space,
                                           weight=smooth_w)
        loss.backward()                                                                   # :304
        with torch.no_grad():
            vis, radii = pkg["visibility_filter"], pkg["radii"]
            changed = False
            if strategy is not None:
                strategy.add_regularizer_grads(model)
            elif it < args.densify_until and table is None:                               # :308-318
                densify.add_densification_stats(model, pkg["viewspace_points"], radii)   # :310-311 + stats, one kernel
                if it >= args.densify_from and it % args.densify_every == 0:
                    densify.densify_and_prune(model, args.densify_grad_threshold, 0.005, 5.0, 20)
                    changed = True
            model.optimizer.step()                                                        # :322-324
            model.optimizer.zero_grad(set_to_none=True)
            if table_opt is not None:
                table_opt.step()
                table_opt.zero_grad(set_to_none=True)
            if strategy is not None:
                changed = any(strategy.step(model, it, LR_XYZ))
            f3.after_step(model, it, changed, args.densify_until)
        if it % args.log == 0 or it == 1:
            losses.append((it, float(loss.item()), int(model._xyz.shape[0])))
            extra = "" if feature_term is None else f"  feature L1 {float(feature_term.item()):.5f}"
            log(f"iter {it:5d}  loss {losses[-1][1]:.5f}  gaussians {losses[-1][2]}{extra}")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    config.set_async(True)              # back to the library defaults
    config.set_antialiasing(False)
    config.set_absgrad(False)
    if depth_terms:
        config.set_depth_gradient(False)
    log(f"{args.iters} iterations in {dt:.2f} s = {dt / args.iters * 1e3:.3f} ms/iteration")
    return losses, dt


def default_args(**kw):
    d = dict(gaussians=200_000, iters=300, resolution="512x512", views=12, lambda_dssim=0.2, log=50, densify_from=100,
             densify_every=100, densify_until=10_000, exact=False, torch_adam=False, antialiasing=False, absgrad=False,
             densify_grad_threshold=0.0002, multi_view=0, mcmc=False, cap_max=0, depth_weight=0.0, depth_loss="l1", filter3d=False,
             normal_weight=0.0, normal_consistency=0.0, distortion_weight=0.0,
             rendered_normal_consistency=0.0, feature_channels=0, depth_smoothness=0.0, smoothness_order=1,
             smoothness_space="depth")
    d.update(kw)
    return SimpleNamespace(**d)


HELP = {
    "filter3d": "the 3D smoothing filter of Mip-Splatting (luciddreamer_amd.filter3d): render the cloud low-passed per Gaussian by "
                "the highest sampling rate of any training camera; recomputed after every change of the set and every 100 "
                "iterations after densification.  Independent of --antialiasing (the 2D Mip filter); Mip-Splatting uses both",
    "mcmc": "MCMC densification (luciddreamer_amd.mcmc.MCMCStrategy) instead of densify_and_prune: dead Gaussians are relocated, "
            "the set grows 5 % per refinement up to --cap-max, a position noise follows every step; no gradient threshold",
    "cap_max": "with --mcmc: the largest number of Gaussians (0: 1.5 x the initial count)",
    "multi_view": "K > 0: one multi-view step of K views per iteration (parallel.ViewBatch with targets) instead of one view; the "
                  "densification statistics come from the step itself (with --absgrad: the absolute gradient's)",
    "absgrad": "densify by the absolute view-space gradient (AbsGS, config.set_absgrad): per-pixel pulls on a Gaussian are summed "
               "by magnitude, so large Gaussians over blurry regions get split; raise --densify-grad-threshold with it",
    "depth_weight": "with --multi-view: > 0 adds depth supervision against the hidden cloud's depth maps with this weight",
    "depth_loss": "the depth term of --depth-weight: l1 (absolute values, loss.depth_l1) or pearson (1 - correlation, "
                  "loss.depth_pearson; the targets are then corrupted by a per-view scale in [0.5, 2] and shift in [-1, 1])",
    "normal_weight": "single-view loop: > 0 holds the rendered depth's normals to the normals of the hidden cloud's depth map "
                     "(normals.normal_loss) with this weight; turns the depth gradient on",
    "normal_consistency": "single-view loop: > 0 adds normals.normal_consistency(depth, median_depth) with this weight "
                          "(return_median=True); the median's side moves the means only",
    "distortion_weight": "> 0 adds W x the mean depth distortion of the view (return_distortion=True, the \"ndc\" mapping of "
                         "2DGS): pulls the layers a ray blends together in depth; with --multi-view inside the step",
    "rendered_normal_consistency": "> 0 adds normals.rendered_normal_consistency(normals, depth) with this weight "
                                   "(return_normals=True): the rendered normal map against the normals of the rendered depth; "
                                   "with --multi-view inside the step",
    "depth_smoothness": "single-view loop: > 0 adds smooth.depth_smoothness(depth, target image) with this weight: the rendered "
                        "depth is held smooth except across image edges; turns the depth gradient on",
    "smoothness_order": "of --depth-smoothness: 1 (differences of neighbours) or 2 (second differences: planes cost nothing)",
    "smoothness_space": "of --depth-smoothness: on the depth itself or on its inverse",
    "feature_channels": "single-view loop: C > 0 renders a [P,C] feature table next to the colour (features=) and trains it, in a "
                        "torch Adam group of its own, with L1 against a fixed seeded [C,3] projection of the target image; the "
                        "term is printed; the set of Gaussians stays fixed (no densification)",
    "densify_grad_threshold": "clone / split threshold on the accumulated view-space gradient norm (reference: 0.0002).  Summed "
                              "magnitudes are larger than the signed norm: with --absgrad use about 4x (0.0008)",
}


CHOICES = {"depth_loss": ("l1", "pearson"), "smoothness_order": (1, 2), "smoothness_space": ("depth", "inverse")}


def make_parser():
    ap = argparse.ArgumentParser()
    for k, v in vars(default_args()).items():
        if isinstance(v, bool):
            ap.add_argument("--" + k.replace("_", "-"), action="store_true", help=HELP.get(k))
        else:
            ap.add_argument("--" + k.replace("_", "-"), type=type(v), default=v, help=HELP.get(k), choices=CHOICES.get(k))
    return ap


if __name__ == "__main__":
    train(make_parser().parse_args())
