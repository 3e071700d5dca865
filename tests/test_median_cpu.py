"""CPU: the reference of the median depth / id outputs alone (tests/median_ref.py on the C oracle's state), and the argument
structs of lr_render_median / lr_median_backward against their ctypes mirrors.  The GPU tests (tests/test_gpu_median.py) rely on
what is asserted here: the walk agrees with the oracle's own final T, it gives the analytic answers, and the share of
threshold-fragile pixels of the two parity inputs stays under the cap."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from luciddreamer_amd import cameras
from tests import helpers as hp, median_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(mr.INPUTS))
def test_a_median_exists_exactly_where_the_final_T_is_below_one_half(name):
    r = mr.box_reference(name)
    final_T = r["st"]["final_T"]
    assert np.array_equal(r["ids"] >= 0, final_T < np.float32(0.5))
    # the outputs' conventions: the depth of the chosen row, 0 where there is none; a chosen row is a rendered one
    has = r["ids"] >= 0
    assert np.array_equal(r["depth"][has], r["st"]["depths"][r["ids"][has]])
    assert not r["depth"][~has].any()
    assert (r["ref"]["radii"][r["ids"][has]] > 0).all()
    print(name, "defined %.1f %%" % (100.0 * has.mean()), "fragile", int(r["fragile"].sum()), "of", has.size,
          "longest list", int((r["st"]["ranges"][:, 1] - r["st"]["ranges"][:, 0]).max()))


@pytest.mark.parametrize("name", mr.PARITY_INPUTS)
def test_the_parity_inputs_have_few_fragile_pixels(name):
    """The condition of the GPU parity test: at most 0.5 % of the pixels may sit on a threshold."""
    r = mr.box_reference(name)
    assert r["fragile"].sum() <= mr.FRAGILE_CAP * r["fragile"].size, int(r["fragile"].sum())
    assert (r["ids"] >= 0).mean() > 0.5                 # ... and the input exercises the walk


def _coaxial(opacities, depths, W=33, H=21):
    """Isotropic Gaussians on the optical axis of the identity camera (the centre pixel of an odd-sized image), front to back."""
    n = len(opacities)
    cloud = dict(means3D=torch.tensor([[0.0, 0.0, z] for z in depths]), scales=torch.full((n, 3), 0.3),
                 rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]] * n), opacities=torch.tensor([[o] for o in opacities]),
                 shs=torch.zeros(n, 16, 3))
    cam = cameras.identity_camera(W, H)
    ref = hp.run_oracle(cloud, cam, 3, torch.zeros(3))
    st = ref["res"].stage()
    return ref, st, mr.walk(st, W, H)


def test_one_gaussian_is_the_median_where_its_alpha_exceeds_one_half():
    ref, st, (ids, depth, _) = _coaxial([0.9], [4.0])
    H, W = ids.shape
    f32 = np.float32
    ys, xs = np.mgrid[0:H, 0:W]
    dx, dy = st["means2D"][0, 0] - xs.astype(f32), st["means2D"][0, 1] - ys.astype(f32)
    a, b, c, op = (f32(v) for v in st["conic_opacity"][0])
    alpha = np.minimum(f32(0.99), op * np.exp(f32(-0.5) * (a * dx * dx + c * dy * dy) - b * dx * dy))
    clear = np.abs(alpha - 0.5) > 1e-6                  # (1 - alpha rounds at alpha = 0.5)
    inside = alpha > 0.5
    assert inside.any() and (~inside).any()
    assert np.array_equal((ids == 0)[clear], inside[clear])
    assert (depth[inside & clear] == st["depths"][0]).all() and st["depths"][0] == f32(4.0)
    assert (ids[~inside & clear] == -1).all() and not depth[~inside & clear].any()


@pytest.mark.parametrize("front_opacity, expected", [(0.4, 1), (0.6, 0)])
def test_two_coaxial_gaussians(front_opacity, expected):
    """Front 0.4 / back 0.9: T = 0.6 behind the front one, the back one takes it below one half; front 0.6: the front one does.
    The expected depth lies strictly between the two surfaces either way -- where there is none."""
    ref, st, (ids, depth, _) = _coaxial([front_opacity, 0.9], [3.0, 5.0])
    H, W = ids.shape
    cy, cx = H // 2, W // 2
    assert st["means2D"][0, 0] == cx and st["means2D"][0, 1] == cy
    assert ids[cy, cx] == expected
    assert depth[cy, cx] == np.float32((3.0, 5.0)[expected])
    assert 3.0 < ref["depth"][0, cy, cx] < 5.0


def test_gradient_reference_puts_each_pixel_on_its_row():
    ids = np.array([[0, 2, 2], [-1, 0, 2]], np.int32)
    G = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    view = np.arange(16, dtype=np.float64)
    g, n, sabs = mr.grad_means3D(ids, G, view, 4)
    assert np.array_equal(n, [2, 0, 3, 0]) and np.array_equal(sabs, [6.0, 0.0, 11.0, 0.0])
    assert np.array_equal(g, np.outer([6.0, 0.0, 11.0, 0.0], [2.0, 6.0, 10.0]))


# ---- the argument structs (the method of tests/test_view_args_cpu.py) ---------------------------------------------------------
@pytest.mark.parametrize("c_name, mirror", [("lr_median_args", "MedianArgs"), ("lr_median_backward_args", "MedianBackwardArgs")])
def test_ctypes_structure_mirrors_the_header(tmp_path, c_name, mirror):
    from luciddreamer_amd import _lib
    S = getattr(_lib, mirror)
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    members = [(f[0], getattr(S, f[0]).offset, getattr(S, f[0]).size) for f in S._fields_]
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
    end = 0                                             # every member is mirrored: the fields tile the struct up to padding
    for n, o, s in members:
        assert 0 <= o - end < 8, n
        end = o + s
    assert 0 <= ctypes.sizeof(S) - end < 8


def test_struct_bytes_and_empty_calls_without_a_device():
    from luciddreamer_amd import _lib, build
    build.build()
    L = _lib.lib()
    for entry, S in ((L.lr_render_median, _lib.MedianArgs), (L.lr_median_backward, _lib.MedianBackwardArgs)):
        assert entry(None) == _lib.LR_ERR_INVALID_ARG
        a = S()
        assert a.struct_bytes == ctypes.sizeof(S)
        for wrong in (0, a.struct_bytes - 8, a.struct_bytes + 8):
            a.struct_bytes = wrong
            assert entry(a) == _lib.LR_ERR_INVALID_ARG, wrong
            assert b"struct_bytes" in L.lr_last_error()
    assert L.lr_median_backward(_lib.MedianBackwardArgs(P=0, width=8, height=8)) == 0          # nothing to do: no device touched
    assert L.lr_render_median(_lib.MedianArgs(P=5, width=8, height=8)) == _lib.LR_ERR_INVALID_ARG
    assert b"scratch buffers" in L.lr_last_error()
