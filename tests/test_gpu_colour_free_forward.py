"""The colour nobody reads is not blended (lr_views_accumulate, render_fwd.hip COLOR = false): a depth-free view of a step driven
by fixed upstream gradients whose out_color[v] the caller does not give runs the forward without the colour channels, and every bit
the step produces stays where it was.  Everything is compared bit for bit (float tensors viewed as int32), on the scenes of
tests/test_gpu_step_invariants.py; lr_last_forward_channels says which kernel the step's last view ran.
"""
import ctypes

import pytest
import torch

from tests.test_gpu_step_invariants import ACC_SHAPES, CAPACITY, H, N_VIEWS, P, W, _assert_same, _bits_equal, _host_array, _scene

gpu = pytest.mark.gpu

ALL = tuple(range(N_VIEWS))


def _step(device, sc, *, color_views=(), depth_views=(), alpha=True, train=False):
    """One step through ViewBatch, three chains.  Returns (what must not depend on the kept images: accumulators, radii, alpha
    images or losses), {view: colour image}, {view: depth image}, channel set of the step's last forward."""
    from luciddreamer_amd import _lib, parallel
    w, h = sc["cams"][0].image_width, sc["cams"][0].image_height
    kw = dict(targets=sc["targets"], depth_targets=sc["depth_targets"], depth_weight=0.5) if train else \
        dict(grad_alphas=sc["grad_alphas"]) if alpha else {}
    if alpha and not train:
        kw["alphas"] = [torch.full((1, h, w), -1.0, device=device) for _ in range(N_VIEWS)]
    batch = parallel.ViewBatch(sc["cams"], None if train else [sc["grad"]] * N_VIEWS, 3, sc["bg"], binning_capacity=CAPACITY,
                               n_streams=3, **kw)
    colors = [torch.full((3, h, w), -1.0, device=device) if v in color_views else None for v in range(N_VIEWS)]
    depths = [torch.full((1, h, w), -1.0, device=device) if v in depth_views else None for v in range(N_VIEWS)]
    radii = [torch.full((P,), -1, dtype=torch.int32, device=device) for _ in range(N_VIEWS)]
    if color_views:
        batch._args.out_color = _host_array(batch, colors)
    if depth_views:
        batch._args.out_depth = _host_array(batch, depths)
    batch._args.out_radii = _host_array(batch, radii)
    acc = {k: torch.zeros((P,) + s, device=device) for k, s in ACC_SHAPES.items()}
    c = sc["cloud"]
    batch.run(c["means3D"], c["opacities"], c["scales"], c["rotations"], c["shs"], acc)
    batch.check()
    out = dict(acc)
    out["radii"] = radii
    if "alphas" in kw:
        out["alpha"] = kw["alphas"]
    if train:
        out["losses"] = batch.losses.clone()
    return (out, {v: t for v, t in enumerate(colors) if t is not None}, {v: t for v, t in enumerate(depths) if t is not None},
            _lib.last_forward_channels())


@pytest.fixture
def knobs():
    from luciddreamer_amd import _lib
    yield _lib.tune_set
    _lib.tune_set("fwd_pair", -1)
    _lib.tune_set("strict", -1)


def _nonzero_gradients(out):
    return all(float(out[k].abs().max()) > 0 for k in ACC_SHAPES)


_PER_VIEW = {}


def _per_view(device, sc, v):
    """(colour, depth) of view v from the per-view operator, rendered once."""
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings, GaussianRasterizer
    from tests import helpers as hp
    key = (id(sc), v)
    if key not in _PER_VIEW:
        cam, c = sc["cams"][v], sc["cloud"]
        tfx, tfy = hp.tan_fov(cam)
        raster = GaussianRasterizer(GaussianRasterizationSettings(cam.image_height, cam.image_width, tfx, tfy, sc["bg"], 1.0,
                                                                  cam.world_view_transform, cam.full_proj_transform, 3,
                                                                  cam.camera_center, False, False))
        with torch.no_grad():
            res = raster(means3D=c["means3D"], means2D=torch.zeros(P, 3, device=device), opacities=c["opacities"], shs=c["shs"],
                         scales=c["scales"], rotations=c["rotations"])
        _PER_VIEW[key] = (res[0].clone(), res[2].clone())
    return _PER_VIEW[key]


# ---- 1. colour off against colour on ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("shape", [0, 2])
@pytest.mark.parametrize("kind", ["band", "box"])
def test_colour_free_forward_leaves_every_bit(hip_device, knobs, kind, shape, strict):
    sc = _scene(hip_device, kind)
    knobs("fwd_pair", shape)
    knobs("strict", 1 if strict else -1)
    on, colors, _, ran_on = _step(hip_device, sc, color_views=ALL)
    off, none, _, ran_off = _step(hip_device, sc)
    assert len(colors) == N_VIEWS and not none
    assert ran_on == "color" and ran_off == "none", (ran_on, ran_off)
    _assert_same(off, on, f"{kind} fwd_pair={shape} strict={strict}")
    assert _nonzero_gradients(on) and any(float(a.max()) > 0 for a in on["alpha"])
    assert all(float(c.min()) >= 0 for c in colors.values())                       # (the images were written: no -1 fill left)


# ---- 2. long lists: checkpoints and c_final of segmented tiles ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [0, 2])
def test_colour_free_forward_writes_checkpoints(hip_device, knobs, shape):
    """3000 Gaussians of the box cloud on the four tiles of a 32 x 32 image: more than 1024 of them are on screen, so at least one
    tile's list is longer than a segment of 256, and the backward's later segments start from the checkpoints and c_final that
    the colour-free kernel's colour-carrying copy of the rounds left."""
    sc = _scene(hip_device, "box", 32, 32, "lookaround")
    knobs("fwd_pair", shape)
    on, _, _, ran_on = _step(hip_device, sc, color_views=ALL)
    off, _, _, ran_off = _step(hip_device, sc)
    assert ran_on == "color" and ran_off == "none", (ran_on, ran_off)
    assert min(int((r > 0).sum()) for r in on["radii"]) > 4 * 256
    _assert_same(off, on, f"fwd_pair={shape}")
    assert _nonzero_gradients(on)


# ---- 3. mixed step ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [0, 2])
def test_mixed_step_colour_for_two_views_of_five(hip_device, knobs, shape):
    sc = _scene(hip_device, "band")
    knobs("fwd_pair", shape)
    want, _, _, _ = _step(hip_device, sc, color_views=ALL)
    got, colors, _, ran = _step(hip_device, sc, color_views=(1, 3))
    assert ran == "none"                                                             # (view 4, the step's last, keeps no image)
    _assert_same(got, want)
    assert sorted(colors) == [1, 3]
    for v, color in colors.items():
        ref = _per_view(hip_device, sc, v)[0]
        assert _bits_equal(color.reshape(-1), ref.reshape(-1)), v
        assert float(ref.max()) > 0


# ---- 4. the training step keeps its colour --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [0, 2])
def test_targets_step_keeps_its_colour(hip_device, knobs, shape):
    """A step with targets (and depth_targets) forms its losses on the blended colour, whether the caller keeps the images or the
    step reads the slot's own: the same losses and gradients, and the colour-carrying kernel."""
    sc = _scene(hip_device, "band")
    knobs("fwd_pair", shape)
    want, colors, _, ran_kept = _step(hip_device, sc, color_views=ALL, train=True)
    got, _, _, ran = _step(hip_device, sc, train=True)
    assert ran_kept == "color+depth" and ran == "color+depth", (ran_kept, ran)
    _assert_same(got, want)
    assert float(want["losses"][:, 0].min()) > 0 and _nonzero_gradients(want)
    assert all(float(c.max()) > 0 for c in colors.values())


# ---- 5. depth kept, colour not ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [0, 2])
def test_views_that_keep_their_depth_carry_the_colour(hip_device, knobs, shape):
    """out_depth for views 1 and 4 and no out_color: no fourth channel set, those two views blend colour and depth (view 4 is the
    step's last forward), the other three neither."""
    sc = _scene(hip_device, "band")
    knobs("fwd_pair", shape)
    want, _, _, _ = _step(hip_device, sc, color_views=ALL)
    got, _, depths, ran = _step(hip_device, sc, depth_views=(1, 4))
    assert ran == "color+depth", ran
    _assert_same(got, want)
    for v, depth in depths.items():
        ref = _per_view(hip_device, sc, v)[1]
        assert _bits_equal(depth.reshape(-1), ref.reshape(-1)), v
        assert float(ref.max()) > 0
    _, _, _, ran = _step(hip_device, sc, depth_views=(1, 3))
    assert ran == "none", ran                                                        # (view 4 keeps nothing in this one)


# ---- 6. the per-view entry points still refuse a NULL out_color ------------------------------------------------------------
def test_per_view_entries_refuse_a_null_out_color():
    """lr_view_forward and lr_forward return their colour: NULL is LR_ERR_INVALID_ARG, in front of the first allocation and the
    first HIP call, with an out_depth and without one."""
    from luciddreamer_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 72)()
    ptr = (ctypes.addressof(buf) + 15) & ~15                                         # non-NULL, aligned, never dereferenced

    @_lib.ALLOC_FN
    def never_called(nbytes, user):
        raise AssertionError("allocator called")

    view = _lib.View(P=100, D=3, M=16, raw=0, background=ptr, width=40, height=24, means3D=ptr, shs=ptr, opacities=ptr, scales=ptr,
                     scale_modifier=1.0, rotations=ptr, viewmatrix=ptr, projmatrix=ptr, campos=ptr, tan_fovx=0.5, tan_fovy=0.5)
    for depth in (ptr, None):
        args = _lib.ForwardArgs(view=view, geom_alloc=never_called, binning_alloc=never_called, img_alloc=never_called,
                                out_color=None, out_depth=depth, radii=ptr, binning_capacity=1000)
        assert L.lr_view_forward(args) == _lib.LR_ERR_INVALID_ARG
        assert b"out_color" in L.lr_last_error()
        rc = L.lr_forward(never_called, None, never_called, None, never_called, None, 100, 3, 16, ptr, 40, 24, ptr, ptr, None, ptr,
                          ptr, 1.0, ptr, None, ptr, ptr, ptr, 0.5, 0.5, 0, None, depth, ptr, 0, 1000, None)
        assert rc == _lib.LR_ERR_INVALID_ARG
        assert b"out_color" in L.lr_last_error()
