"""CPU: the geometry regularisers of the multi-view step and the fused geometry pass, as far as no device is needed -- the argument
structs (lr_geometry_args, lr_geometry_backward_args, lr_views_geom_args) as the host compiler lays them out against
their ctypes mirrors, the checks of the entry points that sit in front of the first HIP call, ViewBatch's argument errors, the
`parts` flags and the shape of `losses` for every combination, and the host-side workspace sizes."""
import ctypes
import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


def _members(S, prefix=""):
    """[(C member expression, offset, size)] of a ctypes struct, nested structs (lr_view) flattened; the members a ctypes base
    class holds are those of the C struct's first member, `base`."""
    out = []
    parent = S.__mro__[1]
    if parent is not ctypes.Structure:
        out += _members(parent, prefix + "base.")
    for f in S._fields_:
        name, typ = f[0], f[1]
        d = getattr(S, name)
        if isinstance(typ, type) and issubclass(typ, ctypes.Structure):
            out += [(prefix + name + "." + n, d.offset + o, s) for n, o, s in _members(typ)]
        else:
            out.append((prefix + name, d.offset, d.size))
    return out


@pytest.mark.parametrize("c_name,mirror", [("lr_geometry_args", "GeometryArgs"), ("lr_geometry_backward_args", "GeometryBackwardArgs"),
                                           ("lr_views_args", "ViewsArgs"), ("lr_views_geom_args", "ViewsGeomArgs")])
def test_ctypes_structures_mirror_the_header(tmp_path, c_name, mirror):
    from luciddreamer_amd import _lib
    S = getattr(_lib, mirror)
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    members = _members(S)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lucid_raster.h"\nint main(void)\n{\n'
                   f'    printf("sizeof %zu\\n", sizeof({c_name}));\n' +
                   "".join(f'    printf("{n} %zu %zu\\n", offsetof({c_name}, {n}), sizeof((({c_name}*)0)->{n}));\n'
                           for n, _, _ in members) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(S)}"
    assert lines[1:1 + len(members)] == [f"{n} {o} {s}" for n, o, s in members]
    # every member of the C struct is mirrored: the fields tile the struct up to alignment padding (< 8 bytes per gap)
    end = 0
    for n, o, s in members:
        assert 0 <= o - end < 8, n
        end = o + s
    assert 0 <= ctypes.sizeof(S) - end < 8


def test_new_members_follow_depth_loss():
    """They lie behind everything lr_views_args holds -- which keeps its layout, depth_loss last -- in a struct of another sizeof,
    so the struct_bytes check tells the two callers apart."""
    from luciddreamer_amd import _lib
    A, G = _lib.ViewsArgs, _lib.ViewsGeomArgs
    assert [f[0] for f in A._fields_][-1] == "depth_loss" and issubclass(G, A)
    assert [f[0] for f in G._fields_] == ["distortion_weight", "distortion_map", "normal_consistency_weight", "out_distortion",
                                          "out_normals"]
    assert G.distortion_map.size == 12 and G.distortion_weight.offset == ctypes.sizeof(A)
    assert all(getattr(G, f[0]).offset == getattr(A, f[0]).offset for f in A._fields_)
    assert ctypes.sizeof(G) > ctypes.sizeof(A)
    assert A(n_views=0).struct_bytes == ctypes.sizeof(A) and G(n_views=0).struct_bytes == ctypes.sizeof(G)


def test_struct_bytes_selects_the_argument_struct(L):
    """sizeof(lr_views_args): the step of today, which does not read behind it; sizeof(lr_views_geom_args): the terms; any other
    value is turned away."""
    from luciddreamer_amd import _lib
    A, G = ctypes.sizeof(_lib.ViewsArgs), ctypes.sizeof(_lib.ViewsGeomArgs)
    for wrong in (A - 8, A + 8, G - 8, G + 8, 0):
        a = _fake_step(**TRAIN)
        a.struct_bytes = wrong
        assert L.lr_views_accumulate(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    # a negative weight behind a struct of the plain size is not read: the call gets as far as its workspace
    a = _fake_step(**dict(TRAIN, distortion_weight=-1.0))
    a.struct_bytes = A
    assert L.lr_views_accumulate(a) == _lib.LR_ERR_INVALID_ARG and b"workspace too small" in L.lr_last_error()
    a.struct_bytes = G
    assert L.lr_views_accumulate(a) == _lib.LR_ERR_INVALID_ARG and b"distortion_weight" in L.lr_last_error()


def test_exports_and_struct_bytes(L):
    from luciddreamer_amd import _lib
    assert {"lr_render_geometry", "lr_geometry_backward"} <= set(_lib.EXPORTS)
    for entry, S in ((L.lr_render_geometry, _lib.GeometryArgs), (L.lr_geometry_backward, _lib.GeometryBackwardArgs)):
        assert entry(None) == _lib.LR_ERR_INVALID_ARG
        a = S(view=_lib.View(P=0, width=8, height=8))
        for wrong in (0, a.struct_bytes - 8, a.struct_bytes + 8):
            a.struct_bytes = wrong
            assert entry(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()


def test_entry_point_checks_in_front_of_the_first_launch(L):
    from luciddreamer_amd import _lib
    assert L.lr_geometry_backward(_lib.GeometryBackwardArgs(view=_lib.View(P=0, width=8, height=8))) == 0       # nothing to do
    assert L.lr_geometry_backward(_lib.GeometryBackwardArgs(view=_lib.View(P=-1, width=8, height=8))) == _lib.LR_ERR_INVALID_ARG
    assert L.lr_render_geometry(_lib.GeometryArgs(view=_lib.View(P=5, width=0, height=8))) == 0
    assert L.lr_render_geometry(_lib.GeometryArgs(view=_lib.View(P=5, width=8, height=8))) == _lib.LR_ERR_INVALID_ARG   # no buffers
    buf = dict(geom_buffer=64, binning_buffer=64, image_buffer=64)
    v = _lib.View(P=5, width=8, height=8, cov3D_precomp=64)
    assert L.lr_render_geometry(_lib.GeometryArgs(view=v, **buf)) == _lib.LR_ERR_INVALID_ARG
    assert b"cov3D_precomp" in L.lr_last_error()
    assert L.lr_geometry_backward(_lib.GeometryBackwardArgs(view=v, **buf)) == _lib.LR_ERR_INVALID_ARG
    assert b"cov3D_precomp" in L.lr_last_error()
    v = _lib.View(P=5, width=8, height=8, scales=64, rotations=64, means3D=64, viewmatrix=64, projmatrix=64)
    assert L.lr_render_geometry(_lib.GeometryArgs(view=v, **buf)) == _lib.LR_ERR_INVALID_ARG and b"required" in L.lr_last_error()
    assert L.lr_render_geometry(_lib.GeometryArgs(view=v, out_distortion=64, out_moments=64, out_normals=64, **buf)) \
        == _lib.LR_ERR_INVALID_ARG and b"required" in L.lr_last_error()                                          # radii, gauss_normals
    assert L.lr_render_geometry(_lib.GeometryArgs(view=v, radii=64, out_distortion=64, out_moments=72, out_normals=64,
                                                  out_gauss_normals=64, **buf)) == _lib.LR_ERR_INVALID_ARG
    assert b"aligned" in L.lr_last_error()
    # the backward: a distortion upstream needs the forward's moments and distortion, dL_dnormals the normals
    need = dict(gauss_normals=64, radii=64, dL_dgauss_normal=64, dL_dmean2D=64, dL_dopacity=64, dL_dmean3D=64, dL_dscale=64,
                dL_drot=64)
    a = _lib.GeometryBackwardArgs(view=v, dL_ddistortion_scalar=0.5, **need, **buf)
    assert L.lr_geometry_backward(a) == _lib.LR_ERR_INVALID_ARG and b"moments" in L.lr_last_error()
    a = _lib.GeometryBackwardArgs(view=v, dL_dnormals=64, **need, **buf)
    assert L.lr_geometry_backward(a) == _lib.LR_ERR_INVALID_ARG and b"normals is required" in L.lr_last_error()
    a = _lib.GeometryBackwardArgs(view=v, dL_ddistortion_scalar=float("nan"), moments=64, distortion=64, **need, **buf)
    assert L.lr_geometry_backward(a) == _lib.LR_ERR_INVALID_ARG and b"finite" in L.lr_last_error()
    a = _lib.GeometryBackwardArgs(view=v, dL_dnormals=64, normals=64, **dict(need, dL_drot=None), **buf)
    assert L.lr_geometry_backward(a) == _lib.LR_ERR_INVALID_ARG and b"dL_drot" in L.lr_last_error()


# ---- lr_views_accumulate --------------------------------------------------------------------------------------------------
def _fake_step(n=2, **fields):
    """tests/test_views_args_cpu.py's fake step: pointers that are non-NULL but never dereferenced on the device."""
    from luciddreamer_amd import _lib
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    arr = (ctypes.c_void_p * n)(*([ptr] * n))
    per_view = ctypes.addressof(arr)
    tans = (ctypes.c_float * n)(*([0.5] * n))
    a = _lib.ViewsGeomArgs(n_views=n, viewmatrices=per_view, projmatrices=per_view, cam_positions=per_view,
                           tan_fovx=ctypes.addressof(tans), tan_fovy=ctypes.addressof(tans), P=100, D=0, M=1, background=ptr,
                           width=16, height=16, means3D=ptr, shs=ptr, opacities=ptr, scales=ptr, rotations=ptr,
                           scale_modifier=1.0, acc_mean2D=ptr, acc_opacity=ptr, acc_mean3D=ptr, acc_sh=ptr, acc_scale=ptr,
                           acc_rot=ptr, workspace=ptr, workspace_bytes=0, binning_capacity=1000, n_streams=2)
    a._keep = (buf, arr, tans)
    for k, v in fields.items():
        if k == "distortion_map":
            v = (ctypes.c_float * 3)(*v)
        setattr(a, k, {"ptr": ptr, "per_view": per_view}.get(v, v) if isinstance(v, str) else v)
    return a


TRAIN = dict(targets="per_view", out_losses="ptr", lambda_dssim=0.2)
REJECTED = {
    "negative_distortion_weight": (dict(TRAIN, distortion_weight=-0.5), b"distortion_weight"),
    "nan_distortion_weight": (dict(TRAIN, distortion_weight=float("nan")), b"distortion_weight"),
    "inf_normal_weight": (dict(TRAIN, normal_consistency_weight=float("inf")), b"normal_consistency_weight"),
    "negative_normal_weight": (dict(TRAIN, normal_consistency_weight=-1.0), b"normal_consistency_weight"),
    "distortion_without_targets": (dict(dL_dpix="per_view", distortion_weight=1.0), b"need targets"),
    "normal_term_without_targets": (dict(dL_dpix="per_view", normal_consistency_weight=1.0), b"need targets"),
    "maps_without_targets": (dict(dL_dpix="per_view", out_normals="per_view"), b"need targets"),
    "nan_map": (dict(TRAIN, distortion_weight=1.0, distortion_map=(0.0, float("nan"), 0.0)), b"distortion_map"),
    "no_acc_rot": (dict(TRAIN, normal_consistency_weight=1.0, acc_rot=None), b"acc_rot"),
    "no_scales": (dict(TRAIN, out_distortion="per_view", scales=None), b"scales"),
    # everything in order: the call gets as far as its workspace, which the fake step does not have
    "workspace": (dict(TRAIN, distortion_weight=1.0, normal_consistency_weight=0.5, distortion_map=(0.0, 1.0, 0.0)),
                  b"workspace too small"),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_rejected_step_arguments_return_invalid_arg_without_a_device(L, case):
    from luciddreamer_amd import _lib
    fields, message = REJECTED[case]
    a = _fake_step(**fields)
    assert L.lr_views_accumulate(a) == _lib.LR_ERR_INVALID_ARG
    assert message in L.lr_last_error(), L.lr_last_error()


def test_workspace_sizes(L):
    """LOSS | 64 is a layout and a larger one; 64 alone, 64 without the colour loss and the values that are no flag are not;
    every value without the flag keeps its size, whatever it was (the geometry part sits behind everything else)."""
    from luciddreamer_amd import _lib
    LOSS, DEPTH, MASK, PEARSON, GEOM = (_lib.LR_VIEWS_LOSS, _lib.LR_VIEWS_DEPTH_LOSS, _lib.LR_VIEWS_MASK_LOSS,
                                        _lib.LR_VIEWS_DEPTH_PEARSON, _lib.LR_VIEWS_GEOM)
    assert GEOM == 64
    au = lambda x: (x + 255) // 256 * 256
    for P, W, H, cap in ((1, 16, 16, 1000), (2000, 70, 45, 60_000), (1_000_000, 1920, 1080, 30_000_000)):
        N = W * H
        images = au(4 * N) + au(16 * N) + au(12 * N) + au(12 * N) + au(12 * N) + au(4 * N)    # D, moments, N, n, dL/dn, dL/ddepth
        per_gauss = au(16 * P) + au(12 * P)
        for n in (1, 2, 4):
            size = lambda parts: L.lr_views_workspace_bytes(P, W, H, cap, n, parts)
            for old in (LOSS, LOSS | DEPTH, LOSS | MASK, LOSS | DEPTH | MASK, LOSS | DEPTH | PEARSON, LOSS | MASK | PEARSON):
                assert size(old) > 0
                grow = size(old | GEOM) - size(old)
                assert grow > 0 and grow % n == 0
                # the maps, the upstream images, two per-Gaussian rows, and the partial sums of the two values
                assert 0 < grow // n - images - per_gauss <= au(16 * N // 64 + 4096), (P, W, H, n, old)
            assert size(GEOM) == 0 and size(GEOM | DEPTH) == 0 and size(LOSS | 32) == 0 and size(LOSS | 8) == 0
            assert size(LOSS | GEOM | 32) == 0 and size(LOSS | GEOM | 128) == 0
            assert size(0) > 0
    buf = (ctypes.c_char * 256)()
    for bad in (GEOM, GEOM | DEPTH, LOSS | GEOM | 32):
        assert L.lr_views_check(ctypes.addressof(buf), 100, 16, 16, 1000, 2, bad, None) == _lib.LR_ERR_INVALID_ARG


# ---- ViewBatch ------------------------------------------------------------------------------------------------------------
def _cams(n, W=32, H=24):
    eye = torch.eye(4)
    return [SimpleNamespace(world_view_transform=eye, full_proj_transform=eye, camera_center=torch.zeros(3), FoVx=1.0, FoVy=0.8,
                            image_width=W, image_height=H) for _ in range(n)]


def test_view_batch_argument_errors():
    from luciddreamer_amd import parallel
    n, W, H = 2, 32, 24
    img, dep = [torch.zeros(3, H, W)] * n, [torch.zeros(1, H, W)] * n
    kw = dict(bg=torch.zeros(3), binning_capacity=1000, sh_degree=0)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="distortion_weight"):
            parallel.ViewBatch(_cams(n, W, H), None, targets=img, distortion_weight=bad, **kw)
        with pytest.raises(ValueError, match="normal_consistency_weight"):
            parallel.ViewBatch(_cams(n, W, H), None, targets=img, normal_consistency_weight=bad, **kw)
    for given in (dict(distortion_weight=1.0), dict(normal_consistency_weight=0.0), dict(distortions=dep), dict(normal_maps=img)):
        with pytest.raises(ValueError, match="go with targets"):
            parallel.ViewBatch(_cams(n, W, H), img, **given, **kw)
    for spelling in ("log", ("ndc", 5.0, 1.0), ("ndc", 0.0, 1.0), 3):
        with pytest.raises(ValueError, match="distortion_map"):
            parallel.ViewBatch(_cams(n, W, H), None, targets=img, distortion_weight=1.0, distortion_map=spelling, **kw)
    with pytest.raises(ValueError, match="distortions: 1 entries"):
        parallel.ViewBatch(_cams(n, W, H), None, targets=img, distortions=dep[:1], **kw)
    with pytest.raises(ValueError, match="normal_maps: every entry"):
        parallel.ViewBatch(_cams(n, W, H), None, targets=img, normal_maps=dep, **kw)
    with pytest.raises(ValueError, match="distortions: every entry"):
        parallel.ViewBatch(_cams(n, W, H), None, targets=img, distortions=[torch.zeros(H, W)] * n, **kw)
    with pytest.raises(ValueError, match="on the HIP device"):              # outputs are the caller's device tensors
        parallel.ViewBatch(_cams(n, W, H), None, targets=img, distortions=dep, **kw)
    with pytest.raises(ValueError, match="on the HIP device"):
        parallel.ViewBatch(_cams(n, W, H), None, targets=img, normal_maps=img, **kw)


def test_view_batch_parts_losses_and_arguments(L):
    from luciddreamer_amd import _lib, parallel
    n, W, H = 3, 32, 24
    img, dep = [torch.zeros(3, H, W)] * n, [torch.zeros(1, H, W)] * n
    kw = dict(bg=torch.zeros(3), binning_capacity=1000, sh_degree=0, targets=img)
    LOSS, DEPTH, MASK, GEOM = _lib.LR_VIEWS_LOSS, _lib.LR_VIEWS_DEPTH_LOSS, _lib.LR_VIEWS_MASK_LOSS, _lib.LR_VIEWS_GEOM
    others = (({}, LOSS, 3), (dict(depth_targets=dep), LOSS | DEPTH, 4), (dict(masks=dep), LOSS | MASK, 5),
              (dict(depth_targets=dep, masks=dep), LOSS | DEPTH | MASK, 5),
              (dict(depth_targets=dep, depth_loss="pearson"), LOSS | DEPTH | _lib.LR_VIEWS_DEPTH_PEARSON, 4))
    for other, parts, cols in others:
        b = parallel.ViewBatch(_cams(n, W, H), None, **kw, **other)
        assert b.parts == parts and tuple(b.losses.shape) == (n, cols) and not b.geom
        # without the arguments the step is passed lr_views_args itself, as before
        assert type(b._args) is _lib.ViewsArgs and b._args.struct_bytes == ctypes.sizeof(_lib.ViewsArgs)
        for geom in (dict(distortion_weight=0.25), dict(normal_consistency_weight=0.5), dict(distortion_weight=0.0),
                     dict(distortion_weight=1.0, normal_consistency_weight=2.0, distortion_map="linear")):
            g = parallel.ViewBatch(_cams(n, W, H), None, **kw, **other, **geom)
            assert g.parts == parts | GEOM and tuple(g.losses.shape) == (n, 7) and g.geom
            assert type(g._args) is _lib.ViewsGeomArgs and g._args.struct_bytes == ctypes.sizeof(_lib.ViewsGeomArgs)
            assert not g._args.out_distortion and not g._args.out_normals
            assert g._args.distortion_weight == geom.get("distortion_weight", 0.0)
            assert g._args.normal_consistency_weight == geom.get("normal_consistency_weight", 0.0)
            assert g.workspace_bytes(100) > b.workspace_bytes(100)
    near, far = 0.5, 40.0
    for spelling, want in (("ndc", _lib.distortion_map_coefficients("ndc")), ("linear", (0.0, 1.0, 0.0)),
                           (("ndc", near, far), (far / (far - near), 0.0, -far * near / (far - near)))):
        g = parallel.ViewBatch(_cams(n, W, H), None, **kw, distortion_weight=1.0, distortion_map=spelling)
        assert list(g._args.distortion_map) == [ctypes.c_float(c).value for c in want]
