"""CPU: the argument struct of the multi-view step.  lr_views_args as the host compiler lays it out against its ctypes mirror
(_lib.ViewsArgs), field by field, and the argument checks of lr_views_accumulate that sit in front of its first HIP call: they
return their codes on a machine without a device."""
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


def test_ctypes_structure_mirrors_the_header(tmp_path):
    from luciddreamer_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    names = [f[0] for f in _lib.ViewsArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lucid_raster.h"\nint main(void)\n{\n'
                   '    printf("sizeof %zu\\n", sizeof(lr_views_args));\n' +
                   "".join(f'    printf("{n} %zu %zu\\n", offsetof(lr_views_args, {n}), sizeof(((lr_views_args*)0)->{n}));\n'
                           for n in names) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(_lib.ViewsArgs)}"
    want = [f"{n} {getattr(_lib.ViewsArgs, n).offset} {getattr(_lib.ViewsArgs, n).size}" for n in names]
    assert lines[1:1 + len(names)] == want
    # every member of the C struct is mirrored: the fields tile the struct up to alignment padding (< 8 bytes per gap)
    end = 0
    for n in names:
        f = getattr(_lib.ViewsArgs, n)
        assert 0 <= f.offset - end < 8, n
        end = f.offset + f.size
    assert 0 <= ctypes.sizeof(_lib.ViewsArgs) - end < 8


def test_struct_bytes_is_checked_before_anything_else(L):
    from luciddreamer_amd import _lib
    assert L.lr_views_accumulate(None) == _lib.LR_ERR_INVALID_ARG
    a = _lib.ViewsArgs(n_views=0)
    assert a.struct_bytes == ctypes.sizeof(_lib.ViewsArgs)
    assert L.lr_views_accumulate(a) == 0                       # nothing to do: no device is touched
    a.P, a.n_views = 0, 3
    assert L.lr_views_accumulate(a) == 0
    for wrong in (0, a.struct_bytes - 8, a.struct_bytes + 8):
        a.struct_bytes = wrong
        assert L.lr_views_accumulate(a) == _lib.LR_ERR_INVALID_ARG, wrong
        assert b"struct_bytes" in L.lr_last_error()


def _fake_step(n=2, **fields):
    """A step of n views whose pointers are non-NULL but never dereferenced on the device: the per-view arrays are real host
    arrays (the library reads their entries), everything else the address of one host buffer."""
    from luciddreamer_amd import _lib
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    arr = (ctypes.c_void_p * n)(*([ptr] * n))
    per_view = ctypes.addressof(arr)
    tans = (ctypes.c_float * n)(*([0.5] * n))
    a = _lib.ViewsArgs(n_views=n, viewmatrices=per_view, projmatrices=per_view, cam_positions=per_view,
                       tan_fovx=ctypes.addressof(tans), tan_fovy=ctypes.addressof(tans), P=100, D=0, M=1, background=ptr,
                       width=16, height=16, means3D=ptr, shs=ptr, opacities=ptr, scales=ptr, rotations=ptr, scale_modifier=1.0,
                       acc_mean2D=ptr, acc_opacity=ptr, acc_mean3D=ptr, acc_sh=ptr, acc_scale=ptr, acc_rot=ptr,
                       workspace=ptr, workspace_bytes=0, binning_capacity=1000, n_streams=2)
    a._keep = (buf, arr, tans)
    for k, v in fields.items():
        setattr(a, k, {"ptr": ptr, "per_view": per_view}.get(v, v) if isinstance(v, str) else v)
    return a


TRAIN = dict(targets="per_view", out_losses="ptr", lambda_dssim=0.2)
REJECTED = {
    # combinations no entry point ever allowed
    "targets_with_dL_dpix": dict(TRAIN, dL_dpix="per_view"),
    "targets_with_dL_ddepth": dict(TRAIN, dL_ddepth="per_view"),
    "targets_with_dL_dalpha": dict(TRAIN, dL_dalpha="per_view"),
    "targets_with_colors_precomp": dict(TRAIN, colors_precomp="ptr"),
    "targets_with_cov3D_precomp": dict(TRAIN, cov3D_precomp="ptr"),
    "targets_with_acc_color": dict(TRAIN, acc_color="ptr"),
    "targets_with_acc_cov3D": dict(TRAIN, acc_cov3D="ptr"),
    "depth_targets_without_targets": dict(dL_dpix="per_view", depth_targets="per_view", depth_weight=1.0),
    "masks_without_targets": dict(dL_dpix="per_view", masks="per_view", alpha_weight=1.0),
    # the checks of the retired per-mode entry points
    "targets_without_out_losses": dict(TRAIN, out_losses=None),
    "negative_depth_weight": dict(TRAIN, depth_targets="per_view", depth_weight=-0.5),
    "nan_depth_weight": dict(TRAIN, depth_targets="per_view", depth_weight=float("nan")),
    "inf_depth_weight": dict(TRAIN, depth_targets="per_view", depth_weight=float("inf")),
    "negative_alpha_weight": dict(TRAIN, masks="per_view", alpha_weight=-1.0),
    "nan_alpha_weight": dict(TRAIN, masks="per_view", alpha_weight=float("nan")),
    "bad_depth_weight_with_masks": dict(TRAIN, masks="per_view", alpha_weight=1.0, depth_targets="per_view", depth_weight=-1.0),
    "no_driver": dict(),
    "capacity_zero": dict(dL_dpix="per_view", binning_capacity=0),
    "no_workspace": dict(dL_dpix="per_view", workspace=None),
    "workspace_too_small": dict(dL_dpix="per_view"),
    "workspace_too_small_train": dict(TRAIN, workspace_bytes=4096),
    "acc_mean2D_missing": dict(dL_dpix="per_view", acc_mean2D=None),
    "acc_opacity_missing": dict(TRAIN, acc_opacity=None),
    "acc_mean3D_missing": dict(dL_dpix="per_view", acc_mean3D=None),
    "viewmatrices_missing": dict(dL_dpix="per_view", viewmatrices=None),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_rejected_arguments_return_invalid_arg_without_a_device(L, case):
    from luciddreamer_amd import _lib
    a = _fake_step(**REJECTED[case])
    assert L.lr_views_accumulate(a) == _lib.LR_ERR_INVALID_ARG
    assert L.lr_last_error()


@pytest.mark.parametrize("which", ["targets", "depth_targets", "masks"])
def test_null_entry_in_a_per_view_input_is_rejected(L, which):
    from luciddreamer_amd import _lib
    a = _fake_step(**dict(TRAIN, depth_targets="per_view", depth_weight=1.0, masks="per_view", alpha_weight=1.0))
    holed = (ctypes.c_void_p * 2)(a.background, None)
    setattr(a, which, ctypes.addressof(holed))
    assert L.lr_views_accumulate(a) == _lib.LR_ERR_INVALID_ARG
    assert b"NULL entry" in L.lr_last_error()


def test_depth_weight_is_ignored_without_depth_targets(L):
    """A mask step without depth targets does not read depth_weight (it fails later, on its workspace, not on the weight)."""
    from luciddreamer_amd import _lib
    a = _fake_step(**dict(TRAIN, masks="per_view", alpha_weight=1.0, depth_weight=float("nan")))
    assert L.lr_views_accumulate(a) == _lib.LR_ERR_INVALID_ARG
    assert b"workspace too small" in L.lr_last_error()


def test_check_rejects_invalid_parts_without_a_device(L):
    from luciddreamer_amd import _lib
    buf = (ctypes.c_char * 256)()
    for bad in (_lib.LR_VIEWS_DEPTH_LOSS, _lib.LR_VIEWS_MASK_LOSS, _lib.LR_VIEWS_LOSS | 8):
        assert L.lr_views_check(ctypes.addressof(buf), 100, 16, 16, 1000, 2, bad, None) == _lib.LR_ERR_INVALID_ARG
    assert L.lr_views_check(None, 100, 16, 16, 1000, 2, 0, None) == _lib.LR_ERR_INVALID_ARG
