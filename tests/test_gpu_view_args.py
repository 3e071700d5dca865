"""GPU: the per-view C ABI through ctypes.  The reference-shaped positional pair (lr_forward / lr_backward) against the struct
entries (lr_view_forward / lr_view_backward) on the same inputs, and the struct entries in raw mode and in depth + alpha + absgrad
mode against the compiled binding -- bit for bit.  Nothing else calls the positional pair.

Scene: 3000 box Gaussians on a 72 x 40 image (both dimensions leave a partial 16-pixel tile), scaled so that at least one tile's
list is longer than 256 instances: the blend backward's 256-position list segments and the R / binning_capacity bound on their
number are inside the comparison."""
import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib
from tests import helpers as hp

pytestmark = pytest.mark.gpu

P, W, H = 3000, 72, 40
AMPLE = 1 << 20                       # async mode: far more tile instances than the scene has
GRADS = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32 if t.element_size() == 4 else np.uint8)


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def scene(hip_device):
    dev = hip_device
    cam, cloud = hp.box_setup(P, W, H, scale_mult=2.0)
    c = cam.to(dev)
    tfx, tfy = hp.tan_fov(cam)
    s = {k: v.to(dev) for k, v in cloud.items()}
    g = torch.Generator().manual_seed(5)
    s.update(bg=torch.tensor([0.1, 0.2, 0.3], device=dev), view=c.world_view_transform.contiguous(),
             proj=c.full_proj_transform.contiguous(), campos=c.camera_center.contiguous(), tfx=tfx, tfy=tfy, dev=dev,
             dL_dpix=torch.randn(3, H, W, generator=g).to(dev), dL_depths=torch.randn(1, H, W, generator=g).to(dev),
             dL_dalpha=torch.randn(1, H, W, generator=g).to(dev),
             # the stored tensors of raw mode: the activations' inverses (rotations deliberately not unit length)
             opacity_raw=torch.logit(s["opacities"]).contiguous(), scaling_raw=torch.log(s["scales"]).contiguous(),
             rotation_raw=(s["rotations"] * 1.7).contiguous(), features_dc=s["shs"][:, :1].contiguous(),
             features_rest=s["shs"][:, 1:].contiguous())
    return s


def _view(s, raw=False, M=16):
    D = 3 if M == 16 else 0
    p = lambda t: t.data_ptr()
    common = dict(P=P, D=D, M=M, raw=int(raw), background=p(s["bg"]), width=W, height=H, means3D=p(s["means3D"]), scale_modifier=1.0,
                  viewmatrix=p(s["view"]), projmatrix=p(s["proj"]), campos=p(s["campos"]), tan_fovx=s["tfx"], tan_fovy=s["tfy"])
    if raw:
        return _lib.View(shs=p(s["features_dc"]), sh_rest=p(s["features_rest"]) if M > 1 else None, opacities=p(s["opacity_raw"]),
                         scales=p(s["scaling_raw"]), rotations=p(s["rotation_raw"]), **common)
    return _lib.View(shs=p(s["shs"]), opacities=p(s["opacities"]), scales=p(s["scales"]), rotations=p(s["rotations"]), **common)


class _Scratch:
    """The three allocator callbacks of a forward: torch byte tensors, kept for the backward."""
    def __init__(self, dev):
        self.t = {}
        self.fns = {}
        for name in ("geom", "binning", "img"):
            def alloc(nbytes, user, name=name):
                self.t[name] = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
                return self.t[name].data_ptr()
            self.fns[name] = _lib.ALLOC_FN(alloc)


def _outputs(dev):
    return dict(color=torch.empty(3, H, W, device=dev), depth=torch.empty(1, H, W, device=dev),
                radii=torch.empty(P, dtype=torch.int32, device=dev))


def _grad_tensors(dev, raw, M, names):
    shape = dict(dL_dmean2D=(P, 3), dL_dmean2D_abs=(P, 3), dL_dconic=(P, 4), dL_dopacity=(P, 1), dL_dcolor=(P, 3), dL_dmean3D=(P, 3),
                 dL_dcov3D=(P, 6), dL_dsh=(P, 1, 3) if raw else (P, M, 3), dL_dsh_rest=(P, M - 1, 3), dL_dscale=(P, 3), dL_drot=(P, 4))
    # a fixed fill: an element the library left unwritten would still compare equal between two runs, but never by accident of
    # what the allocator handed out
    return {n: torch.full(shape[n], 7.0, device=dev) for n in names}


def _check(L, rc):
    assert rc >= 0 or rc == _lib.LR_NUM_RENDERED_ON_DEVICE, (rc, L.lr_last_error())
    return rc


def _struct_pair(s, capacity, raw=False, M=16, depth=False, alpha=False, absgrad=False, conic=True):
    L, dev = _lib.lib(), s["dev"]
    view, sc, out = _view(s, raw, M), _Scratch(dev), _outputs(dev)
    R = _check(L, L.lr_view_forward(_lib.ForwardArgs(
        view=view, geom_alloc=sc.fns["geom"], binning_alloc=sc.fns["binning"], img_alloc=sc.fns["img"],
        out_color=out["color"].data_ptr(), out_depth=out["depth"].data_ptr(), radii=out["radii"].data_ptr(),
        binning_capacity=capacity)))
    names = ["dL_dmean2D", "dL_dopacity", "dL_dmean3D", "dL_dsh", "dL_dscale", "dL_drot"]
    names += (["dL_dsh_rest"] if M > 1 else []) if raw else (["dL_dconic"] if conic else []) + ["dL_dcolor", "dL_dcov3D"]
    names += ["dL_dmean2D_abs"] if absgrad else []
    g = _grad_tensors(dev, raw, M, names)
    _check(L, L.lr_view_backward(_lib.BackwardArgs(
        view=view, R=R, radii=out["radii"].data_ptr(), geom_buffer=sc.t["geom"].data_ptr(), binning_buffer=sc.t["binning"].data_ptr(),
        image_buffer=sc.t["img"].data_ptr(), dL_dpix=s["dL_dpix"].data_ptr(),
        dL_depths=s["dL_depths"].data_ptr() if depth else None, depth_image=out["depth"].data_ptr() if depth else None,
        dL_dalpha=s["dL_dalpha"].data_ptr() if alpha else None, binning_capacity=capacity,
        **{n: t.data_ptr() for n, t in g.items()})))
    torch.cuda.synchronize(dev)
    res = {k: _bits(t) for k, t in {**out, **g}.items()}
    return res, sc


def _positional_pair(s, capacity, dL_depths=None):
    L, dev = _lib.lib(), s["dev"]
    sc, out = _Scratch(dev), _outputs(dev)
    p = lambda t: t.data_ptr()
    R = _check(L, L.lr_forward(sc.fns["geom"], None, sc.fns["binning"], None, sc.fns["img"], None, P, 3, 16, p(s["bg"]), W, H,
                               p(s["means3D"]), p(s["shs"]), None, p(s["opacities"]), p(s["scales"]), 1.0, p(s["rotations"]), None,
                               p(s["view"]), p(s["proj"]), p(s["campos"]), s["tfx"], s["tfy"], 0, p(out["color"]), p(out["depth"]),
                               p(out["radii"]), 0, capacity, None))
    g = _grad_tensors(dev, False, 16, GRADS)
    _check(L, L.lr_backward(P, 3, 16, R, p(s["bg"]), W, H, p(s["means3D"]), p(s["shs"]), None, p(s["scales"]), 1.0, p(s["rotations"]),
                            None, p(s["view"]), p(s["proj"]), p(s["campos"]), s["tfx"], s["tfy"], p(out["radii"]), p(sc.t["geom"]),
                            p(sc.t["binning"]), p(sc.t["img"]), p(s["dL_dpix"]), dL_depths, *[p(g[n]) for n in GRADS], 0, capacity, 0,
                            None))
    torch.cuda.synchronize(dev)
    return {k: _bits(t) for k, t in {**out, **g}.items()}


@pytest.fixture(scope="module")
def struct_default(scene):
    """The struct pair in the default mode, exact and async: each run twice and equal to itself (per-instance gradient slots, no
    float atomics), and the scene really has a list beyond one 256-position segment."""
    res = {}
    for capacity in (0, AMPLE):
        first, sc = _struct_pair(scene, capacity)
        _same(first, _struct_pair(scene, capacity)[0], f"default mode, capacity {capacity}, run twice")
        res[capacity] = first
        N, T = W * H, ((W + 15) // 16) * ((H + 15) // 16)
        off = 2 * ((4 * N + 255) // 256 * 256)                      # csrc/common.h img_layout: final_T, n_contrib, ranges
        ranges = sc.t["img"].cpu().numpy()[off:off + 8 * T].view(np.uint32).reshape(T, 2).astype(np.int64)
        longest = int((ranges[:, 1] - ranges[:, 0]).max())
        print(f"capacity {capacity}: longest tile list {longest}")
        assert longest > 256
    return res


@pytest.mark.parametrize("capacity", [0, AMPLE], ids=["exact", "async"])
def test_positional_pair_gives_the_struct_entries_bits(scene, struct_default, capacity):
    _same(_positional_pair(scene, capacity), struct_default[capacity], "lr_forward + lr_backward against lr_view_*")


def test_lr_backward_ignores_its_dL_depths(scene, struct_default):
    _same(_positional_pair(scene, 0, dL_depths=scene["dL_depths"].data_ptr()), struct_default[0], "lr_backward with dL_depths")


@pytest.mark.parametrize("M", [16, 1])
def test_raw_struct_pair_gives_the_bindings_bits(scene, M):
    from luciddreamer_amd import _C
    s = scene
    got, _ = _struct_pair(s, 0, raw=True, M=M)
    _same(got, _struct_pair(s, 0, raw=True, M=M)[0], f"raw mode M = {M}, run twice")
    rest = s["features_rest"] if M > 1 else None
    D = 3 if M > 1 else 0
    R, color, depth, radii, geom, binning, img = _C.rasterize_gaussians_raw(
        s["bg"], s["means3D"], s["features_dc"], rest, s["opacity_raw"], s["scaling_raw"], s["rotation_raw"], 1.0, s["view"],
        s["proj"], s["tfx"], s["tfy"], H, W, D, s["campos"], False)
    g = _C.rasterize_gaussians_raw_backward(
        s["bg"], s["means3D"], radii, s["features_dc"], rest, s["opacity_raw"], s["scaling_raw"], s["rotation_raw"], 1.0, s["view"],
        s["proj"], s["tfx"], s["tfy"], s["dL_dpix"], D, s["campos"], geom, R, binning, img, False)
    want = dict(color=color, depth=depth, radii=radii, dL_dmean2D=g[0], dL_dmean3D=g[1], dL_dsh=g[2], dL_dopacity=g[4],
                dL_dscale=g[5], dL_drot=g[6])
    if M > 1:
        want["dL_dsh_rest"] = g[3]
    _same(got, {k: _bits(t) for k, t in want.items()}, f"raw mode M = {M} against _C")


def test_depth_alpha_absgrad_struct_pair_gives_the_bindings_bits(scene):
    from luciddreamer_amd import _C
    s = scene
    kw = dict(depth=True, alpha=True, absgrad=True, conic=False)
    got, _ = _struct_pair(s, 0, **kw)
    _same(got, _struct_pair(s, 0, **kw)[0], "depth + alpha + absgrad mode, run twice")
    e = torch.Tensor([])
    R, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
        s["bg"], s["means3D"], e, s["opacities"], s["scales"], s["rotations"], 1.0, e, s["view"], s["proj"], s["tfx"], s["tfy"], H, W,
        s["shs"], 3, s["campos"], False, False)
    g = _C.rasterize_gaussians_backward(
        s["bg"], s["means3D"], radii, e, s["scales"], s["rotations"], 1.0, e, s["view"], s["proj"], s["tfx"], s["tfy"], s["dL_dpix"],
        s["dL_depths"], s["shs"], 3, s["campos"], geom, R, binning, img, False, depth_image=depth, dL_dout_alpha=s["dL_dalpha"],
        absgrad=True)
    want = dict(color=color, depth=depth, radii=radii, dL_dmean2D=g[0], dL_dcolor=g[1], dL_dopacity=g[2], dL_dmean3D=g[3],
                dL_dcov3D=g[4], dL_dsh=g[5], dL_dscale=g[6], dL_drot=g[7], dL_dmean2D_abs=g[8])
    _same(got, {k: _bits(t) for k, t in want.items()}, "depth + alpha + absgrad mode against _C")
