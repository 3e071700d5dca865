"""CPU: the references of the depth distortion output alone (tests/distort_ref.py), and the argument structs of
lr_render_distortion / lr_distortion_backward against their ctypes mirrors.  The GPU tests (tests/test_gpu_distort.py) rely on what
is asserted here: the identities of the definition, the float32 walk's own error against float64 (FWD_ERR, which sets the GPU
bar), the share of threshold-fragile pixels, and that the float32 restatement of the backward's recursion holds GRAD_RTOL."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import distort_ref as dr, helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(dr.INPUTS) + ["posed"]


# ---- the identities of the definition, float64, one pixel at a time -----------------------------------------------------------
def _pixel(seed, n, spread):
    g = torch.Generator().manual_seed(seed)
    alpha = (0.01 + 0.6 * torch.rand(n, generator=g, dtype=torch.float64)).requires_grad_(True)
    m = (0.3 + spread * torch.rand(n, generator=g, dtype=torch.float64)).requires_grad_(True)
    return alpha, m


def _weights(alpha):
    T = torch.cat([torch.ones(1, dtype=alpha.dtype), torch.cumprod(1.0 - alpha, 0)[:-1]])
    return alpha * T, T


def _D_pairs(w, m):
    d = m[:, None] - m[None, :]
    return (torch.tril(w[:, None] * w[None, :], diagonal=-1) * d * d).sum()


@pytest.mark.parametrize("seed, n, spread", [(0, 2, 1.0), (1, 7, 1.0), (2, 40, 0.05), (3, 119, 1.0)])
def test_identities_of_the_definition(seed, n, spread):
    alpha, m = _pixel(seed, n, spread)
    w, T = _weights(alpha)
    D = _D_pairs(w, m)
    g_alpha, g_m = torch.autograd.grad(D, (alpha, m))
    with torch.no_grad():
        # the running-sum form, shifted by the first layer's m
        mt = m - m[0]
        A_prev, M1_prev, M2_prev = (torch.cumsum(x, 0) - x for x in (w, w * mt, w * mt * mt))
        D_run = (w * (mt * mt * A_prev + M2_prev - 2 * mt * M1_prev)).sum()
        assert abs(D_run - D) <= 1e-13 * max(1.0, float(D))
        A, M1, M2 = w.sum(), (w * mt).sum(), (w * mt * mt).sum()
        q = mt * mt * A - 2 * mt * M1 + M2
        assert abs((w * q).sum() - 2 * D) <= 1e-13 * max(1.0, float(D))                 # sum w q = 2 D
        assert torch.allclose(g_m, 2 * w * (mt * A - M1), rtol=0, atol=1e-13)           # dD/dm, and its sum is zero
        assert abs(g_m.sum()) <= 1e-13
        wq = w * q
        S_back = torch.flip(torch.cumsum(torch.flip(wq, [0]), 0), [0]) - wq             # suffix sums, back to front
        S_front = 2 * D - torch.cumsum(wq, 0)                                           # front to back
        for S in (S_back, S_front):
            assert torch.allclose(g_alpha, T * q - S / (1 - alpha), rtol=0, atol=1e-12)
        # shift invariance
        assert abs(_D_pairs(w, m + 1000.0) - D) <= 1e-9 * max(1.0, float(D))


def test_fewer_than_two_layers_have_no_distortion():
    alpha, m = _pixel(5, 1, 1.0)
    w, _ = _weights(alpha)
    assert float(_D_pairs(w, m).detach()) == 0.0


def test_float64_reference_is_shift_invariant_and_its_colour_is_the_oracles():
    cam, cloud, degree, bg = dr.case("thin")
    color, D0, layers, _ = dr.render64(cloud, cam, degree, bg, dr.SHIFT_PAIR[0])
    _, D1, _, _ = dr.render64(cloud, cam, degree, bg, dr.SHIFT_PAIR[1])
    assert float((D0 - D1).abs().max()) <= 1e-9 and float(D0.max()) > 0.1
    ref, st = dr.stage("thin")
    ok = st["fragile"] == 0
    assert np.abs(color.detach().numpy() - ref["color"])[:, ok].max() <= hp.COLOR_ATOL     # the pipeline restated is the pipeline


# ---- the float32 walk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", sorted(dr.MAPS))
@pytest.mark.parametrize("name", NAMES)
def test_float32_walk_against_float64(name, mapping):
    """The measured float32 error, per input and mapping: what FWD_ERR records (the GPU bar is 4 x it)."""
    r = dr.reference(name, mapping)
    ok = ~r["fragile"]
    assert r["fragile"].sum() <= dr.FRAGILE_CAP * r["fragile"].size, int(r["fragile"].sum())
    assert np.array_equal(r["layers32"][ok], r["layers64"][ok])             # the same layers on every non-fragile pixel
    err = float(np.abs(r["D32"].astype(np.float64) - r["D64"])[ok].max())
    print(f'    ("{name}", "{mapping}"): {err:.2e},   # D max {r["D64"].max():.3e}, fragile share {r["fragile"].mean():.4f}, '
          f'most layers {int(r["layers32"].max())}')
    assert (r["D32"] >= 0).all() and (r["D64"] >= -1e-18).all()
    assert not r["D32"][r["layers32"] < 2].any()                            # exact zeros below two layers
    assert dr.FWD_ERR[(name, mapping)] > 0 and err <= dr.FWD_ERR[(name, mapping)], err     # the record is an upper bound of the run
    assert err > 0.25 * dr.FWD_ERR[(name, mapping)]                        # ... and not a generous one


def test_the_shift_is_not_optional():
    """Linear mapping with the cloud pushed to m = z + 1000: unshifted float32 moments lose the answer, shifted ones keep it."""
    _, st = dr.stage("sparse")
    cam = dr.case("sparse")[0]
    W, H = cam.image_width, cam.image_height
    r = dr.reference("sparse", "linear")
    ok = ~r["fragile"]
    plain = dr.walk32(st, W, H, dr.SHIFT_PAIR[1], shift=False)[0]
    shifted = dr.walk32(st, W, H, dr.SHIFT_PAIR[1])[0]
    e_plain = float(np.abs(plain - r["D64"])[ok].max())
    e_shift = float(np.abs(shifted - r["D64"])[ok].max())
    print("unshifted", e_plain, "shifted", e_shift, "D max", float(r["D64"].max()))
    assert e_plain > 0.05 and e_shift < 1e-4


def test_shift_pair_of_the_float32_walk():
    """c0 = 0 against c0 = 1000 on the linear mapping: the float32 walk's own difference, SHIFT_ERR (the GPU pair: 4 x it)."""
    _, st = dr.stage("sparse")
    cam = dr.case("sparse")[0]
    W, H = cam.image_width, cam.image_height
    a = dr.walk32(st, W, H, dr.SHIFT_PAIR[0])[0]
    b = dr.walk32(st, W, H, dr.SHIFT_PAIR[1])[0]
    err = float(np.abs(a - b).max())
    print(f"SHIFT_ERR = {err:.2e}")
    assert dr.SHIFT_ERR > 0 and 0.25 * dr.SHIFT_ERR < err <= dr.SHIFT_ERR


def test_facts_of_the_inputs():
    longest = {n: int((dr.stage(n)[1]["ranges"][:, 1] - dr.stage(n)[1]["ranges"][:, 0]).max()) for n in ("sparse", "dense", "small")}
    assert longest == {"sparse": 313, "dense": 1963, "small": 273}          # every one crosses the 256-entry staging round
    assert int(dr.reference("dense", "ndc")["layers32"].max()) == 108
    thin = dr.reference("thin", "ndc")["layers32"]
    counts = np.bincount(thin.ravel())
    print("thin: pixels by layer count", counts)
    assert counts[0] > 100 and counts[1] > 100 and counts[2:].sum() > 100   # pixels with 0, 1 and >= 2 layers
    wide = dr.stage("wide")[0]["radii"]
    assert (wide > 32).sum() > 50                                           # Gaussians over many tiles


# ---- the float32 restatement of the backward's recursion ----------------------------------------------------------------------
@pytest.mark.parametrize("mapping", sorted(dr.MAPS))
@pytest.mark.parametrize("name", ["sparse", "dense", "wide", "posed"])
def test_float32_backward_holds_the_gradient_bar(name, mapping):
    """Front to back (the kernel's direction) at the screen-space level against float64 autograd: within GRAD_RTOL of each
    tensor's largest entry.  The other direction is printed next to it."""
    cam, cloud, degree, bg = dr.case(name)
    W, H, P = cam.image_width, cam.image_height, cloud["means3D"].shape[0]
    r = dr.reference(name, mapping)
    _, st = dr.stage(name)
    coef = dr.coefficients(mapping)
    res = {d: dr.backward32(st, W, H, coef, r["G"].numpy(), r["D32"], r["mom32"], P, direction=d) for d in ("front", "back")}
    for k in ("px", "py", "conic", "op", "z"):
        ref = r["mid"][k]
        scale = float(np.abs(ref).max())
        errs = {d: float(np.abs(res[d][k].astype(np.float64) - ref).max()) / scale for d in res}
        print(name, mapping, k, "front %.2e back %.2e of max |g| = %.3e" % (errs["front"], errs["back"], scale))
        assert scale > 0 and errs["front"] <= hp.GRAD_RTOL, (k, errs)


# ---- the argument structs (the method of tests/test_median_cpu.py) ------------------------------------------------------------
@pytest.mark.parametrize("c_name, mirror", [("lr_distortion_args", "DistortionArgs"),
                                            ("lr_distortion_backward_args", "DistortionBackwardArgs")])
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


def test_exports_struct_bytes_and_empty_calls_without_a_device():
    from luciddreamer_amd import _lib, build
    build.build()
    assert {"lr_render_distortion", "lr_distortion_backward"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    for entry, S in ((L.lr_render_distortion, _lib.DistortionArgs), (L.lr_distortion_backward, _lib.DistortionBackwardArgs)):
        assert entry(None) == _lib.LR_ERR_INVALID_ARG
        a = S()
        assert a.struct_bytes == ctypes.sizeof(S)
        for wrong in (0, a.struct_bytes - 8, a.struct_bytes + 8):
            a.struct_bytes = wrong
            assert entry(a) == _lib.LR_ERR_INVALID_ARG, wrong
            assert b"struct_bytes" in L.lr_last_error()
    assert L.lr_distortion_backward(_lib.DistortionBackwardArgs(view=_lib.View(P=0, width=8, height=8))) == 0     # nothing to do
    assert L.lr_render_distortion(_lib.DistortionArgs(P=5, width=8, height=8)) == _lib.LR_ERR_INVALID_ARG
    assert b"scratch buffers" in L.lr_last_error()
    b = _lib.DistortionBackwardArgs(view=_lib.View(P=5, width=8, height=8), geom_buffer=64, binning_buffer=64, image_buffer=64)
    assert L.lr_distortion_backward(b) == _lib.LR_ERR_INVALID_ARG             # required pointers are checked before any use
    assert b"required" in L.lr_last_error()


def test_map_coefficients():
    from luciddreamer_amd._lib import distortion_map_coefficients as coef
    assert coef("linear") == (0.0, 1.0, 0.0)
    assert coef("ndc") == coef(("ndc", 0.2, 100.0)) == pytest.approx(dr.MAPS["ndc"])
    c0, c1, c2 = coef(("ndc", 0.5, 20.0))
    assert c0 + c2 / 0.5 == pytest.approx(0.0) and c0 + c2 / 20.0 == pytest.approx(1.0) and c1 == 0.0
    with pytest.raises(ValueError):
        coef("log")
