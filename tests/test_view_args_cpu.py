"""CPU: the argument structs of the per-view entries.  lr_view, lr_forward_args and lr_backward_args as the host compiler lays
them out against their ctypes mirrors (_lib.View, ForwardArgs, BackwardArgs), field by field, and the argument checks of
lr_view_forward / lr_view_backward that sit in front of their first HIP call: they return their codes on a machine without a
device."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


def _members(struct, prefix=""):
    """(C member path, offset, size) of every leaf member, the nested lr_view flattened."""
    out = []
    for f in struct._fields_:
        d = getattr(struct, f[0])
        if isinstance(f[1], type) and issubclass(f[1], ctypes.Structure):
            out += [(prefix + f[0] + "." + n, d.offset + o, s) for n, o, s in _members(f[1])]
        else:
            out.append((prefix + f[0], d.offset, d.size))
    return out


@pytest.mark.parametrize("c_name, mirror", [("lr_view", "View"), ("lr_forward_args", "ForwardArgs"),
                                            ("lr_backward_args", "BackwardArgs")])
def test_ctypes_structure_mirrors_the_header(tmp_path, c_name, mirror):
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


def _ptr():
    """A non-NULL, 16-byte aligned host address that the checks never dereference."""
    buf = (ctypes.c_float * 72)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


_BUF, PTR = _ptr()


ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)         # _lib.ALLOC_FN (ctypes caches the type)
NO_FN = ALLOC_FN()


@ALLOC_FN
def _never_called(nbytes, user):                       # the checks run in front of the first allocation
    raise AssertionError("allocator called")


def _resolve(fields):
    return {k: (PTR if v == "ptr" else PTR + 4 if v == "ptr+4" else v) for k, v in fields.items()}


def _fake_view(raw, **fields):
    from luciddreamer_amd import _lib
    v = dict(P=100, D=3, M=16, raw=raw, background=PTR, width=40, height=24, means3D=PTR, shs=PTR, opacities=PTR, scales=PTR,
             scale_modifier=1.0, rotations=PTR, viewmatrix=PTR, projmatrix=PTR, campos=PTR, tan_fovx=0.5, tan_fovy=0.5)
    if raw:
        v["sh_rest"] = PTR
    v.update(_resolve(fields))
    return _lib.View(**v)


def _fake_forward(raw=0, view=None, **fields):
    from luciddreamer_amd import _lib
    a = dict(geom_alloc=_never_called, binning_alloc=_never_called, img_alloc=_never_called, out_color=PTR, out_depth=PTR, radii=PTR)
    a.update(_resolve(fields))
    return _lib.ForwardArgs(view=_fake_view(raw, **(view or {})), **a)


def _fake_backward(raw=0, view=None, **fields):
    from luciddreamer_amd import _lib
    a = dict(R=1000, radii=PTR, geom_buffer=PTR, binning_buffer=PTR, image_buffer=PTR, dL_dpix=PTR, dL_dmean2D=PTR, dL_dopacity=PTR,
             dL_dmean3D=PTR, dL_dsh=PTR, dL_dscale=PTR, dL_drot=PTR)
    if raw:
        a["dL_dsh_rest"] = PTR
    a.update(_resolve(fields))
    return _lib.BackwardArgs(view=_fake_view(raw, **(view or {})), **a)


def test_struct_bytes_and_null_are_checked_before_anything_else(L):
    from luciddreamer_amd import _lib
    for entry, S in ((L.lr_view_forward, _lib.ForwardArgs), (L.lr_view_backward, _lib.BackwardArgs)):
        assert entry(None) == _lib.LR_ERR_INVALID_ARG
        assert b"struct_bytes" in L.lr_last_error()
        a = S()                                         # everything else NULL / 0: only struct_bytes can be named
        assert a.struct_bytes == ctypes.sizeof(S)
        for wrong in (0, a.struct_bytes - 8, a.struct_bytes + 8):
            a.struct_bytes = wrong
            assert entry(a) == _lib.LR_ERR_INVALID_ARG, wrong
            assert b"struct_bytes" in L.lr_last_error()


def test_backward_of_an_empty_cloud_returns_zero(L):
    from luciddreamer_amd import _lib
    assert L.lr_view_backward(_lib.BackwardArgs()) == 0                              # P == 0: no device is touched
    assert L.lr_view_backward(_fake_backward(view=dict(P=0), dL_dpix=None, geom_buffer=None)) == 0
    assert L.lr_view_backward(_fake_backward(raw=1, view=dict(P=0))) == 0


# case: (forward arguments, view fields, a piece of the message): every check that forward_core and the raw forward entry had,
# then the combinations the positional entries could not express
FORWARD_REJECTED = {
    "negative_P": (dict(), dict(P=-1), b"must be positive"),
    "zero_width": (dict(), dict(width=0), b"must be positive"),
    "zero_height": (dict(), dict(height=0), b"must be positive"),
    "no_geom_alloc": (dict(geom_alloc=NO_FN), dict(), b"allocator callbacks"),
    "no_binning_alloc": (dict(binning_alloc=NO_FN), dict(), b"allocator callbacks"),
    "no_img_alloc": (dict(img_alloc=NO_FN), dict(), b"allocator callbacks"),
    "no_background": (dict(), dict(background=None), b"are required"),
    "no_viewmatrix": (dict(), dict(viewmatrix=None), b"are required"),
    "no_out_color": (dict(out_color=None), dict(), b"are required"),
    "no_out_depth": (dict(out_depth=None), dict(), b"are required"),
    "no_means3D": (dict(), dict(means3D=None), b"means3D/opacities/radii"),
    "no_opacities": (dict(), dict(opacities=None), b"means3D/opacities/radii"),
    "no_radii": (dict(radii=None), dict(), b"means3D/opacities/radii"),
    "no_colour_input": (dict(), dict(shs=None), b"For non-RGB"),
    "no_covariance_input": (dict(), dict(scales=None), b"scales+rotations or cov3D_precomp"),
    "rotations_missing": (dict(), dict(rotations=None), b"scales+rotations or cov3D_precomp"),
    "sh_degree_too_high": (dict(), dict(D=4, M=25), b"SH degree"),
    "sh_degree_exceeds_M": (dict(), dict(D=3, M=9), b"SH degree"),
    "negative_capacity": (dict(binning_capacity=-1), dict(), b"binning_capacity"),
    "capacity_too_large": (dict(binning_capacity=1 << 32), dict(), b"binning_capacity"),
    "raw_without_features_rest": (dict(raw=1), dict(sh_rest=None), b"raw mode needs"),
    "raw_without_opacity": (dict(raw=1), dict(opacities=None), b"raw mode needs"),
    "raw_M_zero": (dict(raw=1), dict(M=0, D=0, sh_rest=None), b"must be >= 1"),
    # new
    "raw_with_colors_precomp": (dict(raw=1), dict(colors_precomp="ptr"), b"colors_precomp"),
    "raw_with_cov3D_precomp": (dict(raw=1), dict(cov3D_precomp="ptr"), b"cov3D_precomp"),
    "raw_with_prefiltered": (dict(raw=1, prefiltered=1), dict(), b"prefiltered"),
    "activated_with_sh_rest": (dict(), dict(sh_rest="ptr"), b"sh_rest"),
}


@pytest.mark.parametrize("case", sorted(FORWARD_REJECTED))
def test_forward_rejects_without_a_device(L, case):
    from luciddreamer_amd import _lib
    args, view, message = FORWARD_REJECTED[case]
    assert L.lr_view_forward(_fake_forward(view=view, **args)) == _lib.LR_ERR_INVALID_ARG
    assert message in L.lr_last_error()


# every check that the backward entries and backward_core had (all in front of the step accumulator and the first HIP call), then
# the new combinations
BACKWARD_REJECTED = {
    "dL_depths_without_depth_image": (dict(dL_depths="ptr"), dict(), b"dL_depths needs"),
    "raw_dL_depths_without_depth_image": (dict(raw=1, dL_depths="ptr"), dict(), b"dL_depths needs"),
    "raw_without_features_rest": (dict(raw=1), dict(sh_rest=None), b"raw mode needs features_dc"),
    "raw_without_opacity": (dict(raw=1), dict(opacities=None), b"raw mode needs features_dc"),
    "raw_without_scaling": (dict(raw=1), dict(scales=None), b"raw mode needs features_dc"),
    "raw_without_dL_dfeatures_dc": (dict(raw=1, dL_dsh=None), dict(), b"raw mode needs dL_dfeatures_dc"),
    "raw_without_dL_dfeatures_rest": (dict(raw=1, dL_dsh_rest=None), dict(), b"raw mode needs dL_dfeatures_dc"),
    "no_geom_buffer": (dict(geom_buffer=None), dict(), b"scratch buffers"),
    "no_binning_buffer": (dict(binning_buffer=None), dict(), b"scratch buffers"),
    "no_image_buffer": (dict(image_buffer=None), dict(), b"scratch buffers"),
    "no_dL_dpix": (dict(dL_dpix=None), dict(), b"are required"),
    "no_dL_dmean2D": (dict(dL_dmean2D=None), dict(), b"are required"),
    "no_dL_dopacity": (dict(dL_dopacity=None), dict(), b"are required"),
    "no_dL_dmean3D": (dict(raw=1, dL_dmean3D=None), dict(), b"are required"),
    "colors_precomp_without_dL_dcolor": (dict(), dict(shs=None, colors_precomp="ptr"), b"dL_dcolor is required"),
    "cov3D_precomp_without_dL_dcov3D": (dict(dL_dscale=None, dL_drot=None), dict(scales=None, rotations=None, cov3D_precomp="ptr"),
                                        b"dL_dcov3D is required"),
    "scales_without_dL_dscale": (dict(dL_dscale=None), dict(), b"dL_dscale/dL_drot"),
    "scales_without_dL_drot": (dict(dL_drot=None), dict(), b"dL_dscale/dL_drot"),
    "shs_without_dL_dsh": (dict(dL_dsh=None), dict(), b"dL_dsh is required"),
    "misaligned_dL_dmean2D": (dict(dL_dmean2D="ptr+4"), dict(), b"16-byte aligned"),
    "misaligned_dL_dconic": (dict(dL_dconic="ptr+4"), dict(), b"16-byte aligned"),
    "misaligned_dL_dmean2D_abs": (dict(dL_dmean2D_abs="ptr+4"), dict(), b"16-byte aligned"),
    "raw_misaligned_dL_dsh_rest": (dict(raw=1, dL_dsh_rest="ptr+4"), dict(), b"16-byte aligned"),
    "misaligned_accumulated_dL_drot": (dict(dL_drot="ptr+4", accumulate_mask=1 << 8), dict(), b"16-byte aligned"),
    # new
    "raw_with_colors_precomp": (dict(raw=1, dL_dcolor="ptr"), dict(colors_precomp="ptr"), b"colors_precomp"),
    "raw_with_cov3D_precomp": (dict(raw=1, dL_dcov3D="ptr"), dict(cov3D_precomp="ptr"), b"cov3D_precomp"),
    "activated_with_sh_rest": (dict(), dict(sh_rest="ptr"), b"sh_rest"),
    "activated_with_dL_dsh_rest": (dict(dL_dsh_rest="ptr"), dict(), b"dL_dsh_rest"),
}


@pytest.mark.parametrize("case", sorted(BACKWARD_REJECTED))
def test_backward_rejects_without_a_device(L, case):
    from luciddreamer_amd import _lib
    args, view, message = BACKWARD_REJECTED[case]
    assert L.lr_view_backward(_fake_backward(view=view, **args)) == _lib.LR_ERR_INVALID_ARG
    assert message in L.lr_last_error()


def test_the_reference_shaped_pair_reaches_the_same_checks(L):
    """lr_forward / lr_backward fill the structs: a rejected argument set comes back with the struct entries' code and text."""
    from luciddreamer_amd import _lib
    none = NO_FN
    rc = L.lr_forward(none, None, none, None, none, None, 100, 3, 16, PTR, 40, 24, PTR, PTR, None, PTR, PTR, 1.0, PTR, None, PTR, PTR,
                      PTR, 0.5, 0.5, 0, PTR, PTR, PTR, 0, 0, None)
    assert rc == _lib.LR_ERR_INVALID_ARG and b"allocator callbacks" in L.lr_last_error()
    rc = L.lr_backward(100, 3, 16, 1000, PTR, 40, 24, PTR, PTR, None, PTR, 1.0, PTR, None, PTR, PTR, PTR, 0.5, 0.5, PTR, PTR, PTR, PTR,
                       PTR, PTR, PTR + 4, None, PTR, None, PTR, None, PTR, PTR, PTR, 0, 0, 0, None)
    assert rc == _lib.LR_ERR_INVALID_ARG and b"16-byte aligned" in L.lr_last_error()
    # its dL_depths is ignored, not rejected for want of a depth image: an empty cloud returns 0
    assert L.lr_backward(0, 3, 16, 0, PTR, 40, 24, PTR, PTR, None, PTR, 1.0, PTR, None, PTR, PTR, PTR, 0.5, 0.5, PTR, PTR, PTR, PTR,
                         PTR, PTR, PTR, None, PTR, None, PTR, None, PTR, PTR, PTR, 0, 0, 0, None) == 0
