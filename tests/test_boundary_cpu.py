"""CPU: the tensor hand-off ("Tensor hand-off") without a device or the library -- what must be REFUSED before
a pointer leaves Python or the compiled binding.

ViewBatch: every argument whose address the fused multi-view step hands to the library, given in a dtype, size or layout the
kernels would misread.  Each case runs with `_lib.lib` replaced by a function that raises, must end in ValueError, and its valid
twin (float32, right shape) must get as far as that function: the refusal is then the one under test.

Binding: host tensors, P = 4, M = 16, an 8x8 image; per tensor of rasterize_gaussians, rasterize_gaussians_raw and the two backward
bindings one case one element short and one case one row long, each a RuntimeError that names the tensor; the all-valid call ends
in the "HIP device" error that comes after the size checks."""
from types import SimpleNamespace

import pytest
import torch

N, W, H = 3, 32, 24


class _Reached(Exception):
    """Raised by the stub in place of the library: every argument check lies in front of it."""


@pytest.fixture
def library_stub(monkeypatch):
    from luciddreamer_amd import _lib

    def reached():
        raise _Reached()
    monkeypatch.setattr(_lib, "lib", reached)


def _cams(n=N, w=W, h=H, **over):
    eye = torch.eye(4)
    base = dict(world_view_transform=eye, full_proj_transform=eye, camera_center=torch.zeros(3), FoVx=1.0, FoVy=0.8,
                image_width=w, image_height=h)
    return [SimpleNamespace(**dict(base, **over)) for _ in range(n)]


def _rep(t):
    return [t] * N


def _img(*shape, dtype=torch.float32):
    return _rep(torch.zeros(*shape, dtype=dtype))


# case -> (mode, the arguments that differ from the valid call of that mode).  mode "train": targets; "fixed": grad_colors.
def _third_camera_wider():
    cams = _cams()
    cams[2] = _cams(1, w=64)[0]
    return cams


VIEW_BATCH_CASES = {
    # targets
    "targets_float64": ("train", dict(targets=_img(3, H, W, dtype=torch.float64))),
    "targets_uint8": ("train", dict(targets=_img(3, H, W, dtype=torch.uint8))),
    "targets_hwc": ("train", dict(targets=_img(H, W, 3))),
    "targets_half_height": ("train", dict(targets=_img(3, H // 2, W))),
    # grad_colors
    "grad_colors_float64": ("fixed", dict(grad_colors=_img(3, H, W, dtype=torch.float64))),
    "grad_colors_float16": ("fixed", dict(grad_colors=_img(3, H, W, dtype=torch.float16))),
    "grad_colors_one_plane": ("fixed", dict(grad_colors=_img(1, H, W))),
    "grad_colors_hwc": ("fixed", dict(grad_colors=_img(H, W, 3))),
    "grad_colors_not_a_tensor": ("fixed", dict(grad_colors=[torch.zeros(3, H, W), [[0.0]], torch.zeros(3, H, W)])),
    # the planes
    "depth_targets_float64": ("train", dict(depth_targets=_img(1, H, W, dtype=torch.float64))),
    "depth_targets_float16": ("train", dict(depth_targets=_img(1, H, W, dtype=torch.float16))),
    "grad_depths_float64": ("fixed", dict(grad_depths=_img(1, H, W, dtype=torch.float64))),
    "grad_depths_float16": ("fixed", dict(grad_depths=_img(H, W, dtype=torch.float16))),
    "grad_alphas_float64": ("fixed", dict(grad_alphas=_img(1, H, W, dtype=torch.float64))),
    "grad_alphas_float16": ("fixed", dict(grad_alphas=_img(1, H, W, dtype=torch.float16))),
    # the background
    "bg_float64": ("fixed", dict(bg=torch.zeros(3, dtype=torch.float64))),
    "bg_one_element": ("fixed", dict(bg=torch.zeros(1))),
    # the cameras
    "view_matrix_float64": ("fixed", dict(cams=_cams(world_view_transform=torch.eye(4, dtype=torch.float64)))),
    "proj_matrix_3x4": ("fixed", dict(cams=_cams(full_proj_transform=torch.zeros(3, 4)))),
    "camera_centre_4_elements": ("fixed", dict(cams=_cams(camera_center=torch.zeros(4)))),
    "third_camera_wider": ("fixed", dict(cams=_third_camera_wider())),
}
# the valid twin of a case differs from it in nothing but the offending argument: the same optional planes, float32 and [1,H,W]
VALID = {"targets": _img(3, H, W), "grad_colors": _img(3, H, W), "depth_targets": _img(1, H, W), "grad_depths": _img(1, H, W),
         "grad_alphas": _img(1, H, W), "bg": torch.zeros(3), "cams": _cams()}


def _view_batch(mode, **given):
    from luciddreamer_amd import parallel
    kw = dict(cams=VALID["cams"], bg=VALID["bg"], binning_capacity=1000, sh_degree=0,
              grad_colors=VALID["grad_colors"] if mode == "fixed" else None, targets=VALID["targets"] if mode == "train" else None)
    kw.update(given)
    return parallel.ViewBatch(kw.pop("cams"), kw.pop("grad_colors"), **kw)


@pytest.mark.parametrize("case", sorted(VIEW_BATCH_CASES))
def test_view_batch_refuses_what_the_kernels_would_misread(library_stub, case):
    mode, bad = VIEW_BATCH_CASES[case]
    with pytest.raises(ValueError):
        _view_batch(mode, **bad)


@pytest.mark.parametrize("case", sorted(VIEW_BATCH_CASES))
def test_view_batch_valid_twin_reaches_the_library(library_stub, case):
    mode, bad = VIEW_BATCH_CASES[case]
    with pytest.raises(_Reached):
        _view_batch(mode, **{k: VALID[k] for k in bad})


def test_view_batch_copies_layouts_it_does_not_refuse(monkeypatch):
    """Strides and alignment are converted, not refused: a transposed-storage image and a camera matrix one float into a buffer
    arrive at the argument struct as contiguous, 16-byte aligned copies."""
    from luciddreamer_amd import _lib, parallel
    monkeypatch.setattr(_lib, "lib", lambda: SimpleNamespace())
    flat = torch.zeros(17)
    offset = flat[1:].view(4, 4)
    assert offset.is_contiguous()
    cams = _cams(world_view_transform=offset)
    g = _rep(torch.zeros(W, H, 3).permute(2, 1, 0))
    assert g[0].shape == (3, H, W) and not g[0].is_contiguous()
    b = parallel.ViewBatch(cams, g, 0, torch.zeros(3), 1000)
    kept = [t for t in b._keep if isinstance(t, torch.Tensor)]
    assert len(kept) == 4 * N and all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in kept)


# ---- the compiled binding -----------------------------------------------------------------------------------------------------
P, M, IH, IW = 4, 16, 8, 8


def _short(t):
    """One element short: the same values, flat, without the last one."""
    return t.reshape(-1)[:-1].clone()


def _long(t):
    """One row long."""
    return torch.cat([t, t[:1]], dim=0)


def _state():
    """Host stand-ins for what a forward leaves: radii and the two buffers whose size is a host function of P, H, W."""
    from luciddreamer_amd import _lib
    L = _lib.lib()
    return dict(radii=torch.ones(P, dtype=torch.int32), geomBuffer=torch.zeros(L.lr_geom_bytes(P), dtype=torch.uint8),
                binningBuffer=torch.zeros(256, dtype=torch.uint8), imageBuffer=torch.zeros(L.lr_img_bytes(IW, IH), dtype=torch.uint8))


def _activated():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)
    return dict(background=r(3), means3D=r(P, 3), colors_precomp=r(P, 3), opacities=r(P, 1), scales=r(P, 3), rotations=r(P, 4),
                cov3D_precomp=r(P, 6), viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh=r(P, M, 3), campos=r(3),
                dL_dout_color=r(3, IH, IW))


def _raw():
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(*s, generator=g)
    return dict(background=r(3), xyz=r(P, 3), features_dc=r(P, 1, 3), features_rest=r(P, M - 1, 3), opacity=r(P, 1), scaling=r(P, 3),
                rotation=r(P, 4), viewmatrix=torch.eye(4), projmatrix=torch.eye(4), campos=r(3), dL_dout_color=r(3, IH, IW))


def _forward(a):
    from luciddreamer_amd import _C
    return _C.rasterize_gaussians(a["background"], a["means3D"], a["colors_precomp"], a["opacities"], a["scales"], a["rotations"], 1.0,
                                  a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], 0.5, 0.5, IH, IW, a["sh"], 3, a["campos"],
                                  False, False)


def _backward(a):
    from luciddreamer_amd import _C
    s = dict(_state(), **{k: a[k] for k in ("radii",) if k in a})
    return _C.rasterize_gaussians_backward(a["background"], a["means3D"], s["radii"], a["colors_precomp"], a["scales"], a["rotations"],
                                           1.0, a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], 0.5, 0.5, a["dL_dout_color"],
                                           None, a["sh"], 3, a["campos"], s["geomBuffer"], 0, s["binningBuffer"], s["imageBuffer"],
                                           False)


def _raw_forward(a):
    from luciddreamer_amd import _C
    return _C.rasterize_gaussians_raw(a["background"], a["xyz"], a["features_dc"], a["features_rest"], a["opacity"], a["scaling"],
                                      a["rotation"], 1.0, a["viewmatrix"], a["projmatrix"], 0.5, 0.5, IH, IW, 3, a["campos"], False)


def _raw_backward(a):
    from luciddreamer_amd import _C
    s = dict(_state(), **{k: a[k] for k in ("radii",) if k in a})
    return _C.rasterize_gaussians_raw_backward(a["background"], a["xyz"], s["radii"], a["features_dc"], a["features_rest"], a["opacity"],
                                               a["scaling"], a["rotation"], 1.0, a["viewmatrix"], a["projmatrix"], 0.5, 0.5,
                                               a["dL_dout_color"], 3, a["campos"], s["geomBuffer"], 0, s["binningBuffer"],
                                               s["imageBuffer"], False)


_CAMERA = ("background", "viewmatrix", "projmatrix", "campos")
ENTRIES = {
    "forward": (_forward, _activated, ("colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp", "sh") + _CAMERA),
    "backward": (_backward, _activated, ("colors_precomp", "scales", "rotations", "cov3D_precomp", "sh", "dL_dout_color", "radii")
                 + _CAMERA),
    "raw_forward": (_raw_forward, _raw, ("features_dc", "features_rest", "opacity", "scaling", "rotation") + _CAMERA),
    "raw_backward": (_raw_backward, _raw, ("features_dc", "features_rest", "opacity", "scaling", "rotation", "dL_dout_color", "radii")
                     + _CAMERA),
}
SIZE_CASES = [(entry, name, how) for entry, (_, _, names) in ENTRIES.items() for name in names for how in ("short", "long")]


@pytest.mark.parametrize("entry,name,how", SIZE_CASES, ids=[f"{e}-{n}-{h}" for e, n, h in SIZE_CASES])
def test_binding_refuses_a_wrong_element_count(entry, name, how):
    call, valid, _ = ENTRIES[entry]
    a = valid()
    t = a[name] if name != "radii" else _state()["radii"]
    if name == "dL_dout_color" and how == "long":
        # H and W are read from this tensor: one image row more is held against the forward's image state
        from luciddreamer_amd import _lib
        assert _lib.lib().lr_img_bytes(IW, IH + 1) > _lib.lib().lr_img_bytes(IW, IH)
        bad = torch.cat([t, t[:, :1]], dim=1)
    else:
        bad = _short(t) if how == "short" else _long(t)
    assert bad.numel() != t.numel() and bad.dtype == t.dtype
    a[name] = bad
    with pytest.raises(RuntimeError, match=name) as e:
        call(a)
    assert "HIP device" not in str(e.value)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_binding_valid_call_ends_at_the_device_check(entry):
    call, valid, _ = ENTRIES[entry]
    with pytest.raises(RuntimeError, match="HIP device"):
        call(valid())


def test_binding_accepts_flat_opacities_and_empty_placeholders():
    """Equality of element counts: opacities of [P] is as good as [P,1]; the reference's empty placeholders stay 'absent'."""
    a = _activated()
    a.update(opacities=a["opacities"].reshape(P), colors_precomp=torch.Tensor([]), cov3D_precomp=None)
    with pytest.raises(RuntimeError, match="HIP device"):
        _forward(a)
    with pytest.raises(RuntimeError, match="HIP device"):
        _backward(a)
    r = _raw()
    r.update(features_rest=torch.Tensor([]))
    with pytest.raises(RuntimeError, match="HIP device"):
        _raw_forward(r)


def test_binding_keeps_the_means3D_message_first():
    a = _activated()
    a.update(means3D=torch.zeros(P, 4), rotations=torch.zeros(P, 3))
    for call in (_forward, _backward):
        with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):
            call(a)


@pytest.mark.parametrize("entry", ["backward", "raw_backward"])
@pytest.mark.parametrize("name", ["geomBuffer", "imageBuffer"])
@pytest.mark.parametrize("how", ["short", "long"])
def test_binding_refuses_forward_state_of_another_size(monkeypatch, entry, name, how):
    """The forward allocates exactly lr_geom_bytes(P) and lr_img_bytes(W, H): a buffer one byte off is another forward's."""
    import sys
    call, valid, _ = ENTRIES[entry]
    good = _state()
    bad = dict(good, **{name: good[name][:-1].clone() if how == "short" else torch.cat([good[name], good[name][:1]])})
    monkeypatch.setattr(sys.modules[__name__], "_state", lambda: bad)
    with pytest.raises(RuntimeError, match="imageBuffer" if name == "imageBuffer" else "geomBuffer") as e:
        call(valid())
    assert "HIP device" not in str(e.value)


@pytest.mark.parametrize("entry", ["backward", "raw_backward"])
@pytest.mark.parametrize("name", ["radii", "geomBuffer", "binningBuffer", "imageBuffer"])
def test_binding_refuses_forward_state_on_another_device(monkeypatch, entry, name):
    """The forward's state is read in place: it lies where means3D lies (a `meta` tensor stands for 'elsewhere' here)."""
    import sys
    call, valid, _ = ENTRIES[entry]
    good = _state()
    bad = dict(good, **{name: good[name].to("meta")})
    monkeypatch.setattr(sys.modules[__name__], "_state", lambda: bad)
    with pytest.raises(RuntimeError, match=name):
        call(valid())


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_binding_empty_scene_takes_placeholders_in_both_pairs(entry):
    """P == 0 launches nothing: the activated and the raw pair treat the other arguments alike (never looked at)."""
    call, valid, _ = ENTRIES[entry]
    a = valid()
    for k, v in a.items():
        if k in ("means3D", "xyz"):
            a[k] = v[:0]
        elif k not in ("dL_dout_color",) + _CAMERA:
            a[k] = v[:0] if v.dim() else v
    a["background"] = torch.zeros(1)
    a["radii"] = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        call(a)


# ---- the passes behind a forward (_C.py) ------------------------------------------------------------------------------------------
def test_dense_converts_dtype_strides_alignment():
    from luciddreamer_amd import _C
    flat = torch.arange(17, dtype=torch.float64)
    v = flat[1:].view(4, 4).t()
    d = _C._dense(v, torch.device("cpu"))
    assert d.dtype is torch.float32 and d.is_contiguous() and d.data_ptr() % 16 == 0 and d.device.type == "cpu"
    assert torch.equal(d, v.float())
    off = torch.zeros(17)[1:].view(4, 4)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and _C._dense(off, torch.device("cpu")).data_ptr() % 16 == 0
    aligned = torch.zeros(4, 4)
    assert _C._dense(aligned, torch.device("cpu")).data_ptr() == aligned.data_ptr()          # the common case copies nothing


@pytest.mark.parametrize("case", ["radii_int64", "ids_int64", "ids_strided", "radii_elsewhere", "ids_elsewhere", "geom_elsewhere",
                                  "acc_elsewhere", "view_12_elements", "upstream_short"])
def test_median_backward_refuses_before_the_library(library_stub, case):
    """radii and median_ids are read in place as int32 on the device of the forward's buffers; `meta` stands for another device."""
    from luciddreamer_amd import _C
    a = dict(geom=torch.zeros(64, dtype=torch.uint8), binning=torch.zeros(64, dtype=torch.uint8), img=torch.zeros(64, dtype=torch.uint8),
             radii=torch.ones(P, dtype=torch.int32), ids=torch.zeros(IH, IW, dtype=torch.int32), dL=torch.zeros(1, IH, IW),
             view=torch.eye(4), acc=None)
    refusal = r"median_backward: |Buffer must be a contiguous tensor on"
    with pytest.raises(Exception) as e:            # the valid twin passes every check: it ends where the HIP stream is asked for
        _C.median_backward(a["geom"], a["binning"], a["img"], a["radii"], a["ids"], a["dL"], a["view"])
    import re
    assert not isinstance(e.value, _Reached) and not re.search(refusal, str(e.value)), e.value
    a.update({"radii_int64": dict(radii=a["radii"].long()), "ids_int64": dict(ids=a["ids"].long()),
              "ids_strided": dict(ids=torch.zeros(IH, 2 * IW, dtype=torch.int32)[:, ::2]),
              "radii_elsewhere": dict(radii=a["radii"].to("meta")), "ids_elsewhere": dict(ids=a["ids"].to("meta")),
              "geom_elsewhere": dict(geom=a["geom"].to("meta")), "acc_elsewhere": dict(acc=torch.zeros(P, 3, device="meta")),
              "view_12_elements": dict(view=torch.zeros(3, 4)), "upstream_short": dict(dL=torch.zeros(IH * IW - 1))}[case])
    with pytest.raises(RuntimeError, match=refusal):
        _C.median_backward(a["geom"], a["binning"], a["img"], a["radii"], a["ids"], a["dL"], a["view"], accumulate_into=a["acc"])
