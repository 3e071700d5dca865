"""GPU: the tensor hand-off ("Tensor hand-off") -- every entry that turns a torch tensor into a pointer is fed the
same values in another LAYOUT and must return the same bits as its twin, the call with contiguous, 16-byte aligned float32 clones:

    cols      wide[:, :k] of a [rows, k + 1] buffer (NaN in the spare column)
    colmajor  storage transposed, shape kept
    offset    a contiguous view one float into a flat buffer: data_ptr() % 16 == 4
    expanded  stride 0: a constant opacity, a grey background from one element, the upstream gradient of .sum()

and upstream gradients as autograd itself produces them (a loss on image.permute(1, 2, 0)).  torch.equal is a condition, not a
tolerance: a layout must not change a bit.  The twin is anchored once per module: to the float64 oracle at the bars of
tests/test_gpu_parity.py, and to itself (the same call twice gives the same bits -- without that the layout cases prove nothing).

Scene: hp.box_setup with P = 257 (odd, one past a 256-thread group, every segment a non-multiple of 16 bytes), SH degree 3, a
40 x 24 image (the width is no multiple of the tile), a non-zero background, synthetic.upstream_grad, three rotate360 views for
the multi-view step.  Refusals on the device use tensors that are too LARGE only: a missing check shows as a failed assertion,
never as an access outside an allocation (the too-small side of the same `!=` is tests/test_boundary_cpu.py's)."""
import math

import pytest
import torch

from luciddreamer_amd import cameras, config, synthetic
from tests import helpers as hp

pytestmark = pytest.mark.gpu

P, W, H, DEG, CAP = 257, 40, 24, 3, 400_000
BG = torch.tensor([0.1, 0.3, 0.2])
LAYOUTS = ("cols", "colmajor", "offset")
NAN = float("nan")


def lay(t, how):
    """The values of t in another layout (module docstring); spare storage holds NaN."""
    t = t.detach()
    if how == "offset":
        buf = t.new_full((t.numel() + 1,), NAN) if t.is_floating_point() else t.new_zeros(t.numel() + 1)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    if t.dim() < 2 or (how == "colmajor" and t.transpose(0, -1).is_contiguous()):
        buf = t.new_full((2 * t.numel(),), NAN) if t.is_floating_point() else t.new_zeros(2 * t.numel())
        v = buf[::2].view(t.shape) if t.dim() < 2 else buf[::2].unflatten(0, t.shape)
        v.copy_(t)
    elif how == "cols":
        wide = t.new_full(tuple(t.shape[:-1]) + (t.shape[-1] + 1,), NAN)         # one spare column behind the last dimension
        v = wide[..., :-1]
        v.copy_(t)
    else:
        v = t.transpose(0, -1).contiguous().transpose(0, -1)
    assert v.shape == t.shape and not v.is_contiguous() and torch.equal(v, t)
    return v


def twin_of(t):
    return None if t is None else t.detach().clone(memory_format=torch.contiguous_format)


def same(got, want, what=""):
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k in want:
        a, b = got[k], want[k]
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            assert a.shape == b.shape and torch.equal(a, b), (what, k, float((a.double() - b.double()).abs().max()))


@pytest.fixture(scope="module", autouse=True)
def depth_gradient_on():
    """On for the whole module (the module-scoped twins are computed under it too): a gradient of the depth output is honoured."""
    config.set_depth_gradient(True)
    yield
    config.set_depth_gradient(False)


@pytest.fixture(scope="module")
def scene(hip_device):
    from oracle import torch_oracle
    cam, cloud = hp.box_setup(P, W, H)
    dev = hip_device
    g = torch.Generator().manual_seed(9)
    t = {k: v.to(dev) for k, v in cloud.items()}
    t["colors_precomp"] = torch.rand(P, 3, generator=g).to(dev)
    t["cov3D_precomp"] = torch_oracle.cov3d_from_scale_rot(cloud["scales"].double(), 1.0, cloud["rotations"].double()).float().to(dev)
    cam_d = cam.to(dev)
    t.update(bg=BG.to(dev), viewmatrix=cam_d.world_view_transform, projmatrix=cam_d.full_proj_transform, campos=cam_d.camera_center)
    # the stored domain of the same cloud, quaternions un-normalised (tests/test_gpu_raw.py)
    raw = dict(xyz=t["means3D"], features_dc=t["shs"][:, :1, :].contiguous(), features_rest=t["shs"][:, 1:, :].contiguous(),
               opacity=torch.logit(t["opacities"]), scaling=torch.log(t["scales"]),
               rotation=t["rotations"] * (0.5 + 1.5 * torch.rand(P, 1, generator=g).to(dev)))
    ups = dict(color=synthetic.upstream_grad(H, W).to(dev))
    for i, (k, c) in enumerate((("depth", 1), ("alpha", 1), ("median", 1), ("normals", 3), ("distortion", 1))):
        ups[k] = torch.randn(c, H, W, generator=torch.Generator().manual_seed(40 + i)).to(dev)
    cams = [c.to(dev) for c in cameras.rotate360_path(W, H, n_views=30)[:3]]
    return dict(cam=cam, cloud=cloud, t=t, raw=raw, ups=ups, cams=cams, dev=dev)


# ---- the operator ----------------------------------------------------------------------------------------------------------------
SH_REP = ("means3D", "opacities", "scales", "rotations", "shs")
PRE_REP = ("means3D", "opacities", "colors_precomp", "cov3D_precomp")
RAW_REP = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
CAMERA = ("bg", "viewmatrix", "projmatrix", "campos")
OUT_NAMES = {"compiled": ("color", "radii", "depth", "alpha"),
             "python": ("color", "radii", "depth", "alpha", "median", "median_ids", "normals", "distortion"),
             "python_pre": ("color", "radii", "depth", "alpha", "median", "median_ids", "distortion")}
OUT_NAMES["raw"] = OUT_NAMES["python"]
OUT_NAMES["compiled_pre"] = OUT_NAMES["compiled"]
ENTRIES = ("compiled", "python", "raw")


def run_operator(entry, t, ups, mode="explicit"):
    """One forward + backward through `entry`; t: {name: device tensor in any layout}; ups: {output: upstream gradient}.
    mode: "explicit" (torch.autograd.backward with ups as they are), "sum" (the loss is the plain sum of the outputs: autograd's
    expanded ones) or "permute" (a loss on out.permute(1, 2, 0): autograd's permuted strides).  Returns every output and gradient."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd import rasterizer
    base = entry.split("_")[0]
    rep = RAW_REP if base == "raw" else PRE_REP if entry.endswith("_pre") else SH_REP
    leaf = {k: t[k].detach().requires_grad_(True) for k in rep}
    m2d = torch.zeros(P, 3, device=leaf[rep[0]].device, requires_grad=True)
    rs = GaussianRasterizationSettings(H, W, math.tan(0.5 * CAM_FOV[0]), math.tan(0.5 * CAM_FOV[1]), t["bg"], 1.0, t["viewmatrix"],
                                       t["projmatrix"], DEG, t["campos"], False, base == "python")
    names = OUT_NAMES[entry]
    extra = dict(return_alpha=True)
    if base != "compiled":
        extra.update(return_median=True, return_distortion=True, return_normals="normals" in names)
    if base == "raw":
        outs = rasterizer.rasterize_gaussians_raw(leaf["xyz"], m2d, leaf["features_dc"], leaf["features_rest"], leaf["opacity"],
                                                  leaf["scaling"], leaf["rotation"], rs, **extra)
    else:
        outs = GaussianRasterizer(rs)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"], shs=leaf.get("shs"),
                                      colors_precomp=leaf.get("colors_precomp"), scales=leaf.get("scales"),
                                      rotations=leaf.get("rotations"), cov3D_precomp=leaf.get("cov3D_precomp"), **extra)
    assert len(outs) == len(names)
    out = dict(zip(names, outs))
    diff = [k for k in names if k in ups]
    if mode == "explicit":
        torch.autograd.backward([out[k] for k in diff], [ups[k] for k in diff])
    elif mode == "sum":
        sum(out[k].sum() for k in diff).backward()
    else:
        sum((out[k].permute(1, 2, 0) * ups[k].permute(1, 2, 0).contiguous()).sum() for k in diff).backward()
    res = {k: v.detach().clone() for k, v in out.items()}
    res.update({"d_" + k: (v.grad.detach().clone() if v.grad is not None else None) for k, v in leaf.items()})
    res["d_means2D"] = m2d.grad.detach().clone()
    return res


CAM_FOV = (cameras.identity_camera(W, H).FoVx, cameras.identity_camera(W, H).FoVy)


def op_inputs(scene, entry):
    src = scene["raw"] if entry == "raw" else scene["t"]
    t = {k: src[k] for k in (RAW_REP if entry == "raw" else PRE_REP if entry.endswith("_pre") else SH_REP)}
    t.update({k: scene["t"][k] for k in CAMERA})
    return t


def op_ups(scene, entry):
    return {k: v for k, v in scene["ups"].items() if k in OUT_NAMES[entry]}


@pytest.fixture(scope="module")
def twins(scene, depth_gradient_on):
    """The plain contiguous call of every entry, once per module; the reference of every layout case below."""
    return {e: run_operator(e, {k: twin_of(v) for k, v in op_inputs(scene, e).items()}, op_ups(scene, e))
            for e in ("compiled", "compiled_pre", "python", "python_pre", "raw")}


def test_anchor_the_twin_matches_the_oracle(scene, twins):
    """The plain contiguous call at this shape, held to the float64 oracle at tests/test_gpu_parity.py's bars."""
    g = scene["ups"]["color"].cpu()
    ref = hp.run_oracle(scene["cloud"], scene["cam"], DEG, BG, g)
    hip = hp.run_hip(scene["cloud"], scene["cam"], DEG, BG, scene["dev"], g)
    print(hp.compare_forward(hip, ref))
    print(hp.compare_grads_by_row(hip, ref, P))
    # ... and that call IS the twin every layout case is held to: the compiled entry's forward, bit for bit
    for k in ("color", "radii", "depth"):
        assert torch.equal(twins["compiled"][k].cpu(), torch.from_numpy(hip[k])), k
    assert int((ref["radii"] > 0).sum()) > P // 2            # the scene is on screen


@pytest.mark.parametrize("entry", ["compiled", "compiled_pre", "python", "python_pre", "raw"])
def test_anchor_the_twin_repeats_its_bits(scene, twins, entry):
    again = run_operator(entry, {k: twin_of(v) for k, v in op_inputs(scene, entry).items()}, op_ups(scene, entry))
    same(again, twins[entry], entry)
    assert float(twins[entry]["d_" + ("xyz" if entry == "raw" else "means3D")].abs().max()) > 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("entry", ["compiled", "compiled_pre", "python", "python_pre", "raw"])
def test_operator_inputs_in_another_layout(scene, twins, entry, layout):
    """One argument at a time: every output and every gradient keeps its bits."""
    t = op_inputs(scene, entry)
    names = [k for k in t if not (entry.endswith("_pre") and k in ("means3D", "opacities") + CAMERA)]   # covered by the SH twin
    for name in names:
        got = run_operator(entry, dict(t, **{name: lay(t[name], layout)}), op_ups(scene, entry))
        same(got, twins[entry], f"{entry}: {name} as {layout}")


@pytest.mark.parametrize("entry", ENTRIES)
def test_operator_camera_tensors_on_the_host(scene, twins, entry):
    """The settings' background, matrices and camera centre kept on the host: the forward moves them to the device, and so must
    every pass behind it (median, distortion, normals and their backward passes read the same settings)."""
    t = op_inputs(scene, entry)
    for names in (CAMERA, ("viewmatrix",), ("campos",)):
        got = run_operator(entry, dict(t, **{k: t[k].cpu() for k in names}), op_ups(scene, entry))
        same(got, twins[entry], f"{entry}: {names} on the host")


@pytest.mark.parametrize("entry", ENTRIES)
def test_operator_expanded_inputs(scene, entry):
    """Stride 0: a constant opacity and a grey background from one element."""
    t = op_inputs(scene, entry)
    op = "opacity" if entry == "raw" else "opacities"
    dev = scene["dev"]
    t[op] = torch.full((1, 1), 0.4, device=dev).expand(P, 1)
    t["bg"] = torch.full((1,), 0.35, device=dev).expand(3)
    assert t[op].stride(0) == 0 and t["bg"].stride(0) == 0
    got = run_operator(entry, t, op_ups(scene, entry))
    want = run_operator(entry, {k: twin_of(v) for k, v in t.items()}, op_ups(scene, entry))
    same(got, want, entry)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_upstream_gradients_in_another_layout(scene, twins, entry, layout):
    """Colour, depth, alpha (and behind the Python nodes median, normals, distortion), one at a time."""
    t, ups = op_inputs(scene, entry), op_ups(scene, entry)
    for name in ups:
        got = run_operator(entry, t, dict(ups, **{name: lay(ups[name], layout)}))
        same(got, twins[entry], f"{entry}: dL/d{name} as {layout}")


@pytest.mark.parametrize("entry", ENTRIES)
def test_upstream_gradients_as_autograd_makes_them(scene, twins, entry):
    t, ups = op_inputs(scene, entry), op_ups(scene, entry)
    same(run_operator(entry, t, ups, mode="permute"), twins[entry], f"{entry}: permuted loss")
    ones = {k: torch.ones_like(v) for k, v in ups.items()}
    same(run_operator(entry, t, ones, mode="sum"), run_operator(entry, t, ones), f"{entry}: .sum()")
    expanded = {k: torch.ones(1, 1, 1, device=v.device).expand(v.shape) for k, v in ups.items()}
    same(run_operator(entry, t, expanded), run_operator(entry, t, ones), f"{entry}: expanded ones")


@pytest.mark.parametrize("layout", LAYOUTS + ("expanded",))
def test_median_backward_wrapper(scene, layout):
    """_C.median_backward: dL_dmedian and the view matrix in another layout, write mode and accumulate mode."""
    from luciddreamer_amd import _C
    t, dev = scene["t"], scene["dev"]
    f = _C.rasterize_gaussians(t["bg"], t["means3D"], None, t["opacities"], t["scales"], t["rotations"], 1.0, None, t["viewmatrix"],
                               t["projmatrix"], math.tan(0.5 * CAM_FOV[0]), math.tan(0.5 * CAM_FOV[1]), H, W, t["shs"], DEG,
                               t["campos"], False, False)
    _, _, _, radii, geom, binning, img = f
    _, ids = _C.render_median(geom, binning, img, P, H, W)
    assert int((ids >= 0).sum()) > 0
    g = scene["ups"]["median"] if layout != "expanded" else torch.ones(1, 1, 1, device=dev).expand(1, H, W)
    want = _C.median_backward(geom, binning, img, radii, ids, twin_of(g), t["viewmatrix"])
    assert float(want.abs().max()) > 0
    vary = (lambda x: x) if layout == "expanded" else (lambda x: lay(x, layout))
    assert torch.equal(_C.median_backward(geom, binning, img, radii, ids, vary(g), t["viewmatrix"]), want)
    if layout != "expanded":
        assert torch.equal(_C.median_backward(geom, binning, img, radii, ids, g, lay(t["viewmatrix"], layout)), want)
    acc = torch.zeros(P, 3, device=dev)
    _C.median_backward(geom, binning, img, radii, ids, vary(g), t["viewmatrix"], accumulate_into=acc)
    assert torch.equal(acc, want)


# ---- the multi-view step -----------------------------------------------------------------------------------------------------------
ACC = {"means3D": (P, 3), "means2D": (P, 3), "opacity": (P, 1), "sh": (P, 16, 3), "scales": (P, 3), "rotations": (P, 4)}


def _acc(dev, **shapes):
    return {k: torch.zeros(shapes.get(k, s), device=dev) for k, s in ACC.items()}


def _step(scene, acc=None, params=None, **kw):
    """One ViewBatch step (n_streams = 2) over the scene's three views: every acc bucket, the loss rows and the output maps."""
    from luciddreamer_amd import parallel
    t, dev = scene["t"], scene["dev"]
    grad_colors = kw.pop("grad_colors", None)
    outs = {}
    if "targets" in kw or "grad_depths" in kw:
        outs["depths"] = [torch.zeros(1, H, W, device=dev) for _ in scene["cams"]]
    if "masks" in kw or "grad_alphas" in kw:
        outs["alphas"] = [torch.zeros(1, H, W, device=dev) for _ in scene["cams"]]
    batch = parallel.ViewBatch(scene["cams"], grad_colors, DEG, t["bg"], CAP, n_streams=2, **kw, **outs)
    acc = _acc(dev) if acc is None else acc
    p = dict({k: t[k] for k in SH_REP}, **(params or {}))
    batch.run(p["means3D"], p["opacities"], p["scales"], p["rotations"], p["shs"], acc)
    batch.check()
    res = {"acc_" + k: v.clone() for k, v in acc.items()}
    res["losses"] = batch.losses.clone() if batch.losses is not None else None
    for k, seq in outs.items():
        res.update({f"{k}{i}": v.clone() for i, v in enumerate(seq)})
    return res


def _view_images(scene, seed, c, lo=0.0, hole=0.0):
    out = []
    for i in range(len(scene["cams"])):
        g = torch.Generator().manual_seed(seed + i)
        x = lo + torch.rand(c, H, W, generator=g)
        if hole:
            x = torch.where(torch.rand(c, H, W, generator=g) < hole, torch.zeros_like(x), x)
        out.append(x.to(scene["dev"]) if c == 3 else x[0].to(scene["dev"]))
    return out


def test_view_batch_training_inputs_in_another_layout(scene):
    """targets, depth_targets and masks: the fused training step's three per-view inputs."""
    kw = dict(targets=_view_images(scene, 100, 3), depth_targets=_view_images(scene, 200, 1, lo=2.0, hole=0.25),
              masks=[(m > 0.3).float() for m in _view_images(scene, 300, 1)])
    want = _step(scene, **kw)
    same(_step(scene, **kw), want, "twice")
    assert float(want["acc_means3D"].abs().max()) > 0 and want["losses"].shape == (3, 5) and bool((want["losses"][:, 0] > 0).all())
    for layout in LAYOUTS:
        for name in kw:
            got = _step(scene, **dict(kw, **{name: [lay(x, layout) for x in kw[name]]}))
            same(got, want, f"{name} as {layout}")


def test_view_batch_fixed_gradients_in_another_layout(scene):
    """grad_colors, grad_depths and grad_alphas, and the expanded ones of a .sum() loss."""
    kw = dict(grad_colors=[scene["ups"]["color"] * (1 + i) for i in range(3)],
              grad_depths=[scene["ups"]["depth"] * (1 + i) for i in range(3)],
              grad_alphas=[scene["ups"]["alpha"][0] * (1 + i) for i in range(3)])
    want = _step(scene, **kw)
    same(_step(scene, **kw), want, "twice")
    assert float(want["acc_means3D"].abs().max()) > 0
    for layout in LAYOUTS:
        for name in kw:
            got = _step(scene, **dict(kw, **{name: [lay(x, layout) for x in kw[name]]}))
            same(got, want, f"{name} as {layout}")
    ones = {k: [torch.ones_like(x) for x in v] for k, v in kw.items()}
    expanded = {k: [torch.ones((1,) * x.dim(), device=x.device).expand(x.shape) for x in v] for k, v in kw.items()}
    same(_step(scene, **expanded), _step(scene, **ones), "expanded ones")


def test_view_batch_run_refuses_what_is_too_large(scene):
    """acc['means2D'] of [P,4], rotations of [P+1,4], opacities of [P,2]; a parameter on another device; a misaligned rotation
    gradient.  The valid call next to them runs."""
    from luciddreamer_amd import parallel
    t, dev = scene["t"], scene["dev"]
    g = [scene["ups"]["color"]] * 3
    batch = parallel.ViewBatch(scene["cams"], g, DEG, t["bg"], CAP, n_streams=2)

    def run(acc=None, **over):
        p = dict({k: t[k] for k in SH_REP}, **over)
        batch.run(p["means3D"], p["opacities"], p["scales"], p["rotations"], p["shs"], acc if acc is not None else _acc(dev))
    run()
    batch.check()
    for what, call in (("acc means2D [P,4]", lambda: run(acc=_acc(dev, means2D=(P, 4)))),
                       ("rotations [P+1,4]", lambda: run(rotations=torch.ones(P + 1, 4, device=dev))),
                       ("opacities [P,2]", lambda: run(opacities=torch.ones(P, 2, device=dev) * 0.5)),
                       ("shs [P+1,16,3]", lambda: run(shs=torch.zeros(P + 1, 16, 3, device=dev))),
                       ("acc sh [P,17,3]", lambda: run(acc=_acc(dev, sh=(P, 17, 3)))),
                       ("acc rotations off by 4 bytes", lambda: run(acc=dict(_acc(dev), rotations=lay(torch.zeros(P, 4, device=dev), "offset")))),
                       ("rotations off by 4 bytes", lambda: run(rotations=lay(t["rotations"], "offset")))):
        try:
            call()
        except RuntimeError as e:
            assert "ViewBatch.run" in str(e), what
        else:
            pytest.fail(f"ViewBatch.run took {what}")
    torch.cuda.synchronize(dev)


def test_view_batch_run_refuses_another_device(scene):
    if torch.cuda.device_count() < 2:
        pytest.skip("one HIP device: the other-device refusal needs two")
    from luciddreamer_amd import parallel
    t, dev = scene["t"], scene["dev"]
    batch = parallel.ViewBatch(scene["cams"], [scene["ups"]["color"]] * 3, DEG, t["bg"], CAP, n_streams=2)
    with pytest.raises(RuntimeError, match="ViewBatch.run"):
        batch.run(t["means3D"], t["opacities"].to("cuda:1"), t["scales"], t["rotations"], t["shs"], _acc(dev))


def test_binding_refuses_what_is_too_large_on_the_device(scene):
    from luciddreamer_amd import _C
    t, dev = scene["t"], scene["dev"]
    tf = (math.tan(0.5 * CAM_FOV[0]), math.tan(0.5 * CAM_FOV[1]))
    for name, bad in (("rotations", torch.ones(P + 1, 4, device=dev)), ("opacities", torch.ones(P, 2, device=dev)),
                      ("sh", torch.zeros(P + 1, 16, 3, device=dev)), ("viewmatrix", torch.eye(5, device=dev)[:, :4])):
        a = dict(t, sh=t["shs"])
        a[name] = bad
        with pytest.raises(RuntimeError, match=name):
            _C.rasterize_gaussians(a["bg"], a["means3D"], None, a["opacities"], a["scales"], a["rotations"], 1.0, None, a["viewmatrix"],
                                   a["projmatrix"], tf[0], tf[1], H, W, a["sh"], DEG, a["campos"], False, False)


# ---- fused accumulation into a misaligned .grad ------------------------------------------------------------------------------------
def test_fused_accumulation_declines_a_misaligned_grad(scene):
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from luciddreamer_amd import rasterizer
    t, dev, g = scene["t"], scene["dev"], scene["ups"]["color"]

    def two_views(misaligned):
        leaf = {k: t[k].clone().requires_grad_(True) for k in SH_REP}
        leaf["means2D"] = torch.zeros(P, 3, device=dev, requires_grad=True)
        for k, v in leaf.items():
            v.grad = torch.zeros_like(v)
        if misaligned:
            leaf["scales"].grad = lay(torch.zeros(P, 3, device=dev), "offset")
            assert rasterizer._fusable_grad(leaf["scales"], dev) is None
        fusable = [k for k in leaf if rasterizer._fusable_grad(leaf[k], dev) is not None]
        assert sorted(fusable) == sorted(k for k in leaf if not (misaligned and k == "scales"))
        ptrs = {k: leaf[k].grad.data_ptr() for k in fusable}
        for c in scene["cams"][:2]:
            tfx, tfy = hp.tan_fov(c)
            rs = GaussianRasterizationSettings(H, W, tfx, tfy, t["bg"], 1.0, c.world_view_transform, c.full_proj_transform, DEG,
                                               c.camera_center, False, False)
            color, _, _ = GaussianRasterizer(rs)(means3D=leaf["means3D"], means2D=leaf["means2D"], opacities=leaf["opacities"],
                                                 shs=leaf["shs"], scales=leaf["scales"], rotations=leaf["rotations"])
            (color * g).sum().backward()
        assert all(leaf[k].grad.data_ptr() == p for k, p in ptrs.items())          # still accumulated in place
        return {k: v.grad.detach().clone() for k, v in leaf.items()}

    config.set_fused_grad_accumulation(True)
    try:
        want = two_views(False)
        got = two_views(True)
    finally:
        config.set_fused_grad_accumulation(False)
    assert float(want["scales"].abs().max()) > 0
    same(got, want, "misaligned scales.grad")


# ---- the kernels beside the rasterizer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_filter3d_update_and_apply(scene, layout):
    from luciddreamer_amd import filter3d
    t, raw, dev = scene["t"], scene["raw"], scene["dev"]
    packed = filter3d.pack_cameras(scene["cams"], dev)
    want_f, want_seen = filter3d.compute_filter_3d(t["means3D"], packed, return_seen=True)
    assert bool(want_seen.any()) and float(want_f.max()) > 0
    for a, b in ((lay(t["means3D"], layout), packed), (t["means3D"], lay(packed, layout))):
        f, seen = filter3d.compute_filter_3d(a, b, return_seen=True)
        assert torch.equal(f, want_f) and torch.equal(seen, want_seen)
    gs, go = torch.randn(P, 3, generator=torch.Generator().manual_seed(1)).to(dev), torch.randn(P, 1, generator=torch.Generator().manual_seed(2)).to(dev)

    def run(s, o, f, g_s, g_o, activated):
        s, o = s.detach().requires_grad_(True), o.detach().requires_grad_(True)
        out_s, out_o = filter3d.apply(s, o, f, activated=activated)
        torch.autograd.backward([out_s, out_o], [g_s, g_o])
        return dict(s=out_s.detach(), o=out_o.detach(), ds=s.grad, do=o.grad)
    for activated in (False, True):
        base = (raw["scaling"], raw["opacity"], want_f, gs, go)
        want = run(*base, activated)
        for i in range(5):
            args = list(base)
            args[i] = lay(args[i], layout)
            same(run(*args, activated), want, f"apply argument {i} as {layout}, activated={activated}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_reproject_project_and_lift(scene, layout):
    import numpy as np
    from luciddreamer_amd import reproject
    t = scene["t"]
    f = 0.5 * W / math.tan(0.5 * CAM_FOV[0])
    K, R, T = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]]), np.eye(3), np.zeros((3, 1))
    pts, cols = t["means3D"], t["colors_precomp"]
    want = reproject.project(pts, cols, K, R, T, H, W)
    assert int(want.mask.sum()) > 0
    for a, b in ((lay(pts, layout), cols), (pts, lay(cols, layout)), (pts.t().contiguous(), cols), (lay(pts.t().contiguous(), layout), cols)):
        got = reproject.project(a, b, K, R, T, H, W)
        for name, x, y in zip(want._fields, got, want):
            assert (x is None and y is None) or torch.equal(x, y), (name, layout)
    depth = want.depth.clone() + 1.0
    assert torch.equal(reproject.lift(lay(depth, layout), K, R, T), reproject.lift(depth, K, R, T))


def test_mcmc_relocate_rows_inputs(scene):
    """Non-contiguous parameters and indices are refused (they are moved in place: nothing could be copied back); a contiguous
    view one float into a buffer is taken, and gives the bits of the aligned call."""
    from luciddreamer_amd import mcmc
    raw, dev = scene["raw"], scene["dev"]
    names = dict(xyz="xyz", f_dc="features_dc", f_rest="features_rest", opacity="opacity", scaling="scaling", rotation="rotation")
    dst = torch.arange(0, 20, dtype=torch.int32, device=dev)
    src = torch.arange(100, 120, dtype=torch.int32, device=dev)

    def run(over=None, dst=dst, src=src):
        params = {g: raw[k].clone() for g, k in names.items()}
        params.update(over or {})
        mcmc.relocate_rows(dst, src, params)
        return {g: v.clone() for g, v in params.items()}
    want = run()
    assert not torch.equal(want["xyz"], raw["xyz"])
    for g, k in names.items():
        same(run({g: lay(raw[k], "offset")}), want, f"{g} one float into a buffer")
        for layout in ("cols", "colmajor"):
            v = lay(raw[k], layout)
            if not v.is_contiguous():
                with pytest.raises(RuntimeError, match="contiguous"):
                    run({g: v})
    for bad in (dict(dst=lay(dst, "cols")), dict(src=lay(src, "cols"))):
        with pytest.raises(RuntimeError, match="contiguous"):
            run(**bad)
    same(run(dst=lay(dst, "offset"), src=lay(src, "offset")), want, "indices one word into a buffer")


@pytest.mark.parametrize("layout", LAYOUTS + ("expanded",))
def test_video_frames_to_uint8(scene, layout):
    from luciddreamer_amd.video import frames_to_uint8
    dev = scene["dev"]
    g = torch.Generator().manual_seed(3)
    for shape in ((3, H, W), (2, 3, H, W), (3, 5, 7)):                       # H * W a multiple of 4, and not
        x = (1.4 * torch.rand(*shape, generator=g) - 0.2).to(dev)
        if layout == "expanded":
            x = x[..., :1].expand(shape)
        want = frames_to_uint8(twin_of(x))
        ref = (x.clamp(0, 1) * 255).round().to(torch.uint8).movedim(-3, -1)
        assert torch.equal(want, ref)
        assert torch.equal(frames_to_uint8(x if layout == "expanded" else lay(x, layout)), want)
