"""CPU: the references of the rendered normal map output alone (tests/render_normals_ref.py), and the argument structs of
lr_render_normals / lr_render_normals_backward against their ctypes mirrors.  The GPU tests (tests/test_gpu_render_normals.py) rely
on what is asserted here: the float32 walk's own error against float64 (FWD_ERR, which sets the GPU bar), the share of
threshold-fragile pixels, that no Gaussian of an input sits on the orientation test or on a tie of its scales, that the float32
restatement of the backward's recursion holds GRAD_RTOL, and the hand-checked answers of the crafted cloud."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as hp, render_normals_ref as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the identities of the gradient, float64, one pixel at a time -------------------------------------------------------------
@pytest.mark.parametrize("seed, n", [(0, 1), (1, 7), (2, 119)])
def test_identities_of_the_gradient(seed, n):
    g = torch.Generator().manual_seed(seed)
    alpha = (0.01 + 0.6 * torch.rand(n, generator=g, dtype=torch.float64)).requires_grad_(True)
    nrm = torch.randn(n, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    up = torch.randn(3, generator=g, dtype=torch.float64)
    T = torch.cat([torch.ones(1, dtype=alpha.dtype), torch.cumprod(1.0 - alpha, 0)[:-1]])
    w = alpha * T
    N = (w[:, None] * nrm).sum(dim=0)
    g_alpha, g_n = torch.autograd.grad((N * up).sum(), (alpha, nrm))
    with torch.no_grad():
        c = nrm @ up
        wc = w * c
        S_front = (N * up).sum() - torch.cumsum(wc, 0)                              # front to back
        S_back = torch.flip(torch.cumsum(torch.flip(wc, [0]), 0), [0]) - wc         # suffix sums
        for S in (S_front, S_back):
            assert torch.allclose(g_alpha, T * c - S / (1 - alpha), rtol=0, atol=1e-12)
        assert torch.allclose(g_n, w[:, None] * up[None, :], rtol=0, atol=1e-15)
        assert float(N.norm()) <= float(w.sum() * nrm.norm(dim=1).max()) + 1e-12


# ---- the per-Gaussian normal --------------------------------------------------------------------------------------------------
def test_the_normal_is_the_eigenvector_of_the_smallest_scale():
    """Sigma n = s_k^2 n for the oracle's own covariance: R is the matrix of cov3d_from_scale_rot."""
    from oracle import torch_oracle as to
    _, cloud, _, _ = rn.case("small")
    s, q = cloud["scales"].double(), cloud["rotations"].double()
    c = to.cov3d_from_scale_rot(s, 1.0, q)
    Sig = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], dim=1).reshape(-1, 3, 3)
    k = torch.from_numpy(rn.axis_of(cloud["scales"].numpy()))
    n = rn.quat_matrix(q)[torch.arange(s.shape[0]), :, k]
    sk = s[torch.arange(s.shape[0]), k]
    # (the cloud's quaternions are unit to float32 rounding only, so R^T R = 1 to 1e-7)
    assert torch.allclose((Sig @ n[:, :, None])[:, :, 0], sk[:, None] ** 2 * n, rtol=0, atol=1e-7 * float(s.max()) ** 2)
    assert bool((sk == s.min(dim=1).values).all())


def test_axis_ties_take_the_lowest_index():
    s = np.array([[1, 1, 1], [2, 1, 1], [1, 2, 1], [3, 2, 1], [1, 1, 2], [2, 2, 1]], np.float32)
    assert rn.axis_of(s).tolist() == [0, 1, 0, 2, 0, 2]
    assert rn.axis_of(np.log(s)).tolist() == [0, 1, 0, 2, 0, 2]


@pytest.mark.parametrize("name", rn.NAMES)
def test_no_input_sits_on_the_orientation_test_or_on_a_tie(name):
    """The conditions under which no pixel needs masking for the flip or the axis: asserted on the reference alone."""
    _, cloud, _, _ = rn.case(name)
    r = rn.reference(name)
    vis = r["visible"]
    s = np.sort(cloud["scales"].numpy().astype(np.float64), axis=1)
    gap = float(((s[:, 1] - s[:, 0]) / s[:, 0])[vis].min())
    print(f"{name}: min |n^.p^| = {r['margin'][vis].min():.2e}, smallest relative gap of the two shortest scales {gap:.2e}, "
          f"{int((r['sign'][vis] < 0).sum())} of {int(vis.sum())} flipped")
    assert r["margin"][vis].min() > rn.FLIP_BAND
    assert gap > 0                                                   # no tie (the comparison is exact on inputs either way)
    assert np.array_equal(rn.axis_of(cloud["scales"].log().numpy())[vis], r["k"][vis])      # raw mode picks the same axis
    assert (r["sign"][vis] < 0).any() and (r["sign"][vis] > 0).any() and len(set(r["k"][vis].tolist())) == 3
    # the float32 statement agrees: sign, axis, and the components to float32 rounding
    gn = r["gn32"]
    assert np.array_equal(np.sign(gn[vis, 3]), r["sign"][vis]) and np.array_equal(np.abs(gn[vis, 3]) - 1, r["k"][vis])
    assert np.abs(gn[vis, :3] - r["gn64"][vis]).max() <= 2e-6 and not gn[~vis].any()
    # towards the camera: n . p_view <= 0
    cam = rn.case(name)[0]
    pv = cloud["means3D"].double().numpy() @ cam.world_view_transform.double().numpy()[:3, :3] + cam.world_view_transform.double().numpy()[3, :3]
    assert ((r["gn64"] * pv).sum(axis=1)[vis] < 0).all()


# ---- the float32 walk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rn.NAMES)
def test_float32_walk_against_float64(name):
    """The measured float32 error per input: what FWD_ERR records (the GPU bar is 4 x it)."""
    r = rn.reference(name)
    ok = ~r["fragile"]
    assert r["fragile"].sum() <= rn.FRAGILE_CAP * r["fragile"].size, int(r["fragile"].sum())
    assert np.array_equal(r["layers32"][ok], r["layers64"][ok])             # the same layers on every non-fragile pixel
    err = float(np.abs(r["N32"].astype(np.float64) - r["N64"])[:, ok].max())
    print(f'    "{name}": {err:.2e},   # |N| max {np.linalg.norm(r["N64"], axis=0).max():.3f}, fragile share '
          f'{r["fragile"].mean():.4f}, most layers {int(r["layers32"].max())}')
    assert not r["N32"][:, r["layers32"] == 0].any() and not r["N64"][:, r["layers64"] == 0].any()    # exact zeros without a layer
    assert np.linalg.norm(r["N64"], axis=0).max() <= 1.0 + 1e-9             # |N| <= alpha <= 1
    assert rn.FWD_ERR[name] > 0 and err <= rn.FWD_ERR[name], err            # the record is an upper bound of the run
    assert err > 0.25 * rn.FWD_ERR[name]                                    # ... and not a generous one


def test_float64_colour_is_the_oracles():
    cam, cloud, degree, bg = rn.case("thin")
    color, _, _, _ = rn.render64(cloud, cam, degree, bg)
    ref, st = rn.stage("thin")
    ok = st["fragile"] == 0
    assert np.abs(color.detach().numpy() - ref["color"])[:, ok].max() <= hp.COLOR_ATOL     # the pipeline restated is the pipeline


# ---- the float32 restatement of the backward's recursion ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "dense", "wide", "posed"])
def test_float32_backward_holds_the_gradient_bar(name):
    """Front to back (the kernel's direction) at the screen-space level and for dL/dn against float64 autograd: within GRAD_RTOL of
    each tensor's largest entry."""
    cam, cloud, _, _ = rn.case(name)
    W, H, P = cam.image_width, cam.image_height, cloud["means3D"].shape[0]
    r = rn.reference(name)
    _, st = rn.stage(name)
    res = rn.backward32(st, W, H, r["gn32"], r["G"].numpy(), r["N32"], P)
    for k in ("px", "py", "conic", "op", "n"):
        ref = r["mid"][k]
        scale = float(np.abs(ref).max())
        err = float(np.abs(res[k].astype(np.float64) - ref).max()) / scale
        print(name, k, "front %.2e of max |g| = %.3e" % (err, scale))
        assert scale > 0 and err <= hp.GRAD_RTOL, (k, err)


def test_only_the_rotations_see_the_normal():
    """With alpha's path cut (the upstream reaches N through n alone), scales and means get nothing: the axis and the sign are
    constants."""
    cam, cloud, degree, bg = rn.case("thin")
    _, N, _, inter = rn.render64(cloud, cam, degree, bg)
    g, = torch.autograd.grad((inter["n"] * torch.ones_like(inter["n"])).sum(), inter["leaves"]["rotations"], retain_graph=True)
    assert g.abs().max() > 0
    for k in ("means3D", "scales", "opacities", "means2D"):
        assert torch.autograd.grad(inter["n"].sum(), inter["leaves"][k], allow_unused=True, retain_graph=True)[0] is None


# ---- the crafted cloud --------------------------------------------------------------------------------------------------------
def test_crafted_cloud_against_answers_by_hand():
    cam, cloud, degree, bg, expect = rn.crafted()
    color, N, layers, inter = rn.render64(cloud, cam, degree, bg)
    N, layers, alpha = N.detach().numpy(), layers.numpy(), 2.0 * color.detach().numpy()[0]      # shs = 0: rgb = 0.5, bg = 0
    n = inter["n"].detach().numpy()
    assert inter["k"].tolist() == [expect[i][0] for i in range(6)] == [0, 1, 2, 0, 2, 2]
    for i, (_, want) in expect.items():
        assert np.abs(n[i] - want).max() <= 1e-6, (i, n[i], want)     # (the quaternion is float32)
    assert inter["sign"].tolist()[4:] == [-1.0, 1.0]                  # q = 1: (0, 0, 1) faces away, flipped; the pi turn faces the camera
    assert np.abs(n[4] - n[5]).max() == 0.0
    # every pixel with a layer: N / alpha is the normal of the one Gaussian that owns it (they do not overlap)
    px = inter["px"].detach().numpy().round().astype(int)
    py = inter["py"].detach().numpy().round().astype(int)
    assert int(layers.max()) == 1 and (layers > 0).sum() > 300
    for i in range(6):
        y, x = py[i], px[i]
        assert layers[y, x] == 1 and alpha[y, x] > 0.5
        assert np.abs(N[:, y, x] / alpha[y, x] - expect[i][1]).max() <= 1e-6, i
    # the fronto-parallel discs: (0, 0, -1), the depth normal of the plane z = 4, on all of their pixels
    disc = (layers > 0) & (np.arange(N.shape[1])[:, None] > rn.CRAFT_H // 2) & (np.arange(N.shape[2])[None, :] > 22)
    assert disc.sum() > 100
    assert np.abs(N[0][disc]).max() <= 1e-12 and np.abs(N[1][disc]).max() <= 1e-12
    assert np.abs(N[2][disc] + alpha[disc]).max() <= 1e-12
    # the float32 statement of the normals agrees
    ref = hp.run_oracle(cloud, cam, degree, bg)
    gn = rn.gauss_normals32(cloud["means3D"].numpy(), cloud["scales"].numpy(), cloud["rotations"].numpy(),
                            cam.world_view_transform.numpy(), ref["radii"])
    assert gn[:, 3].tolist() == [s * (k + 1) for s, k in zip(inter["sign"].tolist(), inter["k"].tolist())]
    assert np.abs(gn[:, :3] - n).max() <= 1e-6


# ---- the argument structs (the method of tests/test_distort_cpu.py) -----------------------------------------------------------
@pytest.mark.parametrize("c_name, mirror", [("lr_normals_render_args", "NormalsRenderArgs"),
                                            ("lr_normals_render_backward_args", "NormalsRenderBackwardArgs")])
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
    assert {"lr_render_normals", "lr_render_normals_backward"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    for entry, S in ((L.lr_render_normals, _lib.NormalsRenderArgs), (L.lr_render_normals_backward, _lib.NormalsRenderBackwardArgs)):
        assert entry(None) == _lib.LR_ERR_INVALID_ARG
        a = S()
        assert a.struct_bytes == ctypes.sizeof(S)
        for wrong in (0, a.struct_bytes - 8, a.struct_bytes + 8):
            a.struct_bytes = wrong
            assert entry(a) == _lib.LR_ERR_INVALID_ARG, wrong
            assert b"struct_bytes" in L.lr_last_error()
    assert L.lr_render_normals_backward(_lib.NormalsRenderBackwardArgs(view=_lib.View(P=0, width=8, height=8))) == 0    # nothing to do
    assert L.lr_render_normals(_lib.NormalsRenderArgs(view=_lib.View(P=5, width=8, height=8))) == _lib.LR_ERR_INVALID_ARG
    assert b"scratch buffers" in L.lr_last_error()
    # cov3D_precomp: there is no normal, in either direction, whatever else is given (the check is in front of the first HIP call)
    v = _lib.View(P=5, width=8, height=8, cov3D_precomp=64)
    assert L.lr_render_normals(_lib.NormalsRenderArgs(view=v, geom_buffer=64, binning_buffer=64, image_buffer=64)) == _lib.LR_ERR_INVALID_ARG
    assert b"cov3D_precomp" in L.lr_last_error()
    assert L.lr_render_normals_backward(_lib.NormalsRenderBackwardArgs(view=v, geom_buffer=64, binning_buffer=64, image_buffer=64)) \
        == _lib.LR_ERR_INVALID_ARG
    assert b"cov3D_precomp" in L.lr_last_error()
    # required pointers are checked before any use
    v = _lib.View(P=5, width=8, height=8)
    assert L.lr_render_normals(_lib.NormalsRenderArgs(view=v, geom_buffer=64, binning_buffer=64, image_buffer=64, out_normals=64)) \
        == _lib.LR_ERR_INVALID_ARG
    assert b"required" in L.lr_last_error()
    assert L.lr_render_normals_backward(_lib.NormalsRenderBackwardArgs(view=v, geom_buffer=64, binning_buffer=64, image_buffer=64)) \
        == _lib.LR_ERR_INVALID_ARG
    assert b"required" in L.lr_last_error()


def test_python_refuses_cov3d_precomp_before_any_launch():
    """ValueError from the wrappers and the operator without a device: nothing has been launched when it is raised."""
    from luciddreamer_amd import _C
    from luciddreamer_amd.rasterizer import GaussianRasterizationSettings, rasterize_gaussians
    P = 4
    cov = torch.zeros(P, 6)
    empty = torch.Tensor([])
    with pytest.raises(ValueError, match="cov3D_precomp"):
        _C.render_normals(empty, empty, empty, torch.zeros(P, dtype=torch.int32), None, means3D=torch.zeros(P, 3), scales=empty,
                          rotations=empty, cov3D_precomp=cov)
    rs = GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    with pytest.raises(ValueError, match="cov3D_precomp"):
        rasterize_gaussians(torch.zeros(P, 3), torch.zeros(P, 3), empty, torch.zeros(P, 3), torch.zeros(P, 1), empty, empty, cov, rs,
                            return_normals=True)
