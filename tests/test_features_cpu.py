"""CPU: the references of the N-channel feature map output alone (tests/feature_ref.py), and the argument structs, refusals and
wrappers of lr_render_features / lr_render_features_backward.  The GPU tests (tests/test_gpu_features.py) rely on what is asserted
here: the float32 walk's own error against float64 (FWD_ERR, which sets the GPU bar), the share of threshold-fragile pixels, and
that the float32 restatement of the backward's recursion holds GRAD_RTOL."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import feature_ref as fr, helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the identities of the gradient, float64, one pixel at a time -------------------------------------------------------------
@pytest.mark.parametrize("seed, n, C", [(0, 1, 1), (1, 7, 5), (2, 119, 33)])
def test_identities_of_the_gradient(seed, n, C):
    g = torch.Generator().manual_seed(seed)
    alpha = (0.01 + 0.6 * torch.rand(n, generator=g, dtype=torch.float64)).requires_grad_(True)
    f = torch.randn(n, C, generator=g, dtype=torch.float64).requires_grad_(True)
    up = torch.randn(C, generator=g, dtype=torch.float64)
    T = torch.cat([torch.ones(1, dtype=alpha.dtype), torch.cumprod(1.0 - alpha, 0)[:-1]])
    w = alpha * T
    F = (w[:, None] * f).sum(dim=0)
    g_alpha, g_f = torch.autograd.grad((F * up).sum(), (alpha, f))
    with torch.no_grad():
        c = f @ up
        S_front = (F * up).sum() - torch.cumsum(w * c, 0)                           # front to back
        assert torch.allclose(g_alpha, T * c - S_front / (1 - alpha), rtol=0, atol=1e-11)
        assert torch.allclose(g_f, w[:, None] * up[None, :], rtol=0, atol=1e-15)
        # dL/dalpha is linear in the upstream: the chunks' parts add
        parts = torch.zeros_like(g_alpha)
        for c0 in range(0, C, 4):
            cc = f[:, c0:c0 + 4] @ up[c0:c0 + 4]
            Fg = (F[c0:c0 + 4] * up[c0:c0 + 4]).sum()
            parts += T * cc - (Fg - torch.cumsum(w * cc, 0)) / (1 - alpha)
        assert torch.allclose(g_alpha, parts, rtol=0, atol=1e-11)


# ---- the references ---------------------------------------------------------------------------------------------------------------
def test_the_chunk_width_is_the_shipped_one():
    from luciddreamer_amd import _lib
    src = open(os.path.join(ROOT, "luciddreamer_amd", "csrc", "render_features.hip")).read()
    assert int(re.search(r"constexpr int FTR_K = (\d+);", src).group(1)) == fr.K == _lib.LR_FEATURE_CHUNK >= 16
    assert fr.CHANNELS == (1, 3, 5, fr.K, fr.K + 3, 2 * fr.K + 1)


@pytest.mark.parametrize("name", fr.NAMES)
def test_float32_walk_against_float64(name):
    r = fr.reference(name)
    ok = ~r["fragile"]
    err = float(np.abs(r["F32"].astype(np.float64) - r["F64"])[:, ok].max())
    print(name, "walk32 against render64: %.3e on |F| <= %.3f, %d layers at most" % (err, np.abs(r["F64"]).max(), r["layers32"].max()))
    assert fr.FWD_ERR[name] / 4 <= err <= fr.FWD_ERR[name], (err, fr.FWD_ERR[name])
    assert float(r["feats"].abs().max()) <= 1.0 and r["feats"].shape[1] == fr.C_MAX
    # a pixel without a layer is an exact zero in both
    empty = (r["layers32"] == 0) & ok
    assert empty.any() or name != "thin"             # (the input with pixels of 0, 1 and >= 2 layers)
    assert not r["F32"][:, empty].any() and not r["F64"][:, empty].any()


@pytest.mark.parametrize("name", fr.NAMES)
def test_fragile_share(name):
    share = float(fr.reference(name)["fragile"].mean())
    print(name, "fragile share %.2e" % share)
    assert share <= fr.FRAGILE_CAP


@pytest.mark.parametrize("name", ["sparse", "dense", "wide", "posed"])
def test_float32_backward_holds_the_gradient_bar(name):
    cam, cloud, _, _ = fr.case(name)
    H, W, P = cam.image_height, cam.image_width, cloud["means3D"].shape[0]
    r = fr.reference(name)
    _, st = fr.stage(name)
    feats, G = r["feats"].numpy(), r["G"].numpy()
    res = fr.backward32(st, W, H, feats, G, r["F32"], P)
    ref = fr.screen64(st, W, H, feats, G)
    for k in ("px", "py", "conic", "op", "f"):
        scale = float(np.abs(ref[k]).max())
        err = float(np.abs(res[k].astype(np.float64) - ref[k]).max()) / scale
        print(name, k, "front %.2e of max |g| = %.3e" % (err, scale))
        assert scale > 0 and err <= hp.GRAD_RTOL, (k, err)
    # a Gaussian no pixel blended, and one with radii <= 0, get exact zeros
    assert not res["f"][~r["visible"]].any()
    # the table's own gradient agrees with the leaf-level float64 autograd of the workaround as well
    scale = float(np.abs(r["leaf"]["features"]).max())
    assert float(np.abs(res["f"] - r["leaf"]["features"]).max()) <= hp.GRAD_RTOL * scale


def test_channel_permutation_permutes_the_walk_bitwise():
    cam, _, _, _ = fr.case("sparse")
    _, st = fr.stage("sparse")
    r = fr.reference("sparse")
    perm = np.random.default_rng(3).permutation(fr.C_MAX)
    F, _, _ = fr.walk32(st, cam.image_width, cam.image_height, r["feats"].numpy()[:, perm])
    assert np.array_equal(F.view(np.uint32), r["F32"][perm].view(np.uint32))
    # ... and a slice of the table gives the slice of the planes
    F, _, _ = fr.walk32(st, cam.image_width, cam.image_height, r["feats"].numpy()[:, 3:8])
    assert np.array_equal(F.view(np.uint32), r["F32"][3:8].view(np.uint32))


# ---- the argument structs (the method of tests/test_render_normals_cpu.py) ------------------------------------------------------
@pytest.mark.parametrize("c_name, mirror", [("lr_feature_render_args", "FeatureRenderArgs"),
                                            ("lr_feature_render_backward_args", "FeatureRenderBackwardArgs")])
def test_ctypes_structure_mirrors_the_header(tmp_path, c_name, mirror):
    from luciddreamer_amd import _lib
    S = getattr(_lib, mirror)
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    members = [(f[0], getattr(S, f[0]).offset, getattr(S, f[0]).size) for f in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lucid_raster.h"\nint main(void)\n{\n'
                   f'    printf("sizeof %zu\\n", sizeof({c_name}));\n'
                   '    printf("max %d acc %u\\n", LR_FEATURE_MAX_CHANNELS, LR_ACC_FEATURES);\n' +
                   "".join(f'    printf("{n} %zu %zu\\n", offsetof({c_name}, {n}), sizeof((({c_name}*)0)->{n}));\n'
                           for n, _, _ in members) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(S)}"
    assert lines[1] == f"max {_lib.LR_FEATURE_MAX_CHANNELS} acc {_lib.LR_ACC_FEATURES}"
    assert lines[2:2 + len(members)] == [f"{n} {o} {s}" for n, o, s in members]
    end = 0                                             # every member is mirrored: the fields tile the struct up to padding
    for n, o, s in members:
        assert 0 <= o - end < 8, n
        end = o + s
    assert 0 <= ctypes.sizeof(S) - end < 8


def test_the_new_accumulate_bit_leaves_the_others_alone():
    from luciddreamer_amd import _C, _lib
    assert _lib.LR_ACC_FEATURES == 1 << 9
    assert _lib.LR_ACC_FEATURES not in {1 << b for b in list(_C.ACC_BITS.values()) + list(_C.RAW_ACC_BITS.values())} | {1 << 1, 1 << 31}
    assert _C.ACC_BITS == {"means2D": 0, "opacity": 2, "colors": 3, "means3D": 4, "cov3D": 5, "sh": 6, "scales": 7, "rotations": 8}


def _bwd_args(_lib, **over):
    """A backward argument struct that passes every check (dummy, suitably aligned addresses: nothing is dereferenced in front of
    the first HIP call), with `over` laid over it."""
    v = over.pop("view", None) or _lib.View(P=5, width=8, height=8, means3D=64, viewmatrix=64, projmatrix=64, scales=64, rotations=64)
    f = dict(view=v, geom_buffer=64, binning_buffer=64, image_buffer=64, binning_capacity=100, features=64, channels=8,
             dL_dout_features=64, out_features=64, radii=64, dL_dfeatures=64, workspace=64,
             workspace_bytes=_lib.lib().lr_features_workspace_bytes(100, 8), dL_dmean2D=64, dL_dopacity=64, dL_dmean3D=64,
             dL_dscale=64, dL_drot=64)
    f.update(over)
    return _lib.FeatureRenderBackwardArgs(**f)


def test_exports_refusals_and_empty_calls_without_a_device():
    from luciddreamer_amd import _lib, build
    build.build()
    assert {"lr_render_features", "lr_render_features_backward", "lr_features_workspace_bytes"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    INV = _lib.LR_ERR_INVALID_ARG
    for entry, S in ((L.lr_render_features, _lib.FeatureRenderArgs), (L.lr_render_features_backward, _lib.FeatureRenderBackwardArgs)):
        assert entry(None) == INV
        a = S()
        assert a.struct_bytes == ctypes.sizeof(S)
        for wrong in (0, a.struct_bytes - 8, a.struct_bytes + 8):
            a.struct_bytes = wrong
            assert entry(a) == INV, wrong
            assert b"struct_bytes" in L.lr_last_error()
    fwd = lambda **kw: L.lr_render_features(_lib.FeatureRenderArgs(**dict(dict(
        view=_lib.View(P=5, width=8, height=8), geom_buffer=64, binning_buffer=64, image_buffer=64, features=64, channels=8,
        out_features=64), **kw)))
    bwd = lambda **kw: L.lr_render_features_backward(_bwd_args(_lib, **kw))
    # the channel count
    for call in (fwd, bwd):
        for C in (0, -1, _lib.LR_FEATURE_MAX_CHANNELS + 1):
            assert call(channels=C) == INV, C
            assert b"channels" in L.lr_last_error()
    # P = 0 and empty images: nothing to do, no device needed
    assert bwd(view=_lib.View(P=0, width=8, height=8)) == 0
    assert bwd(view=_lib.View(P=5, width=0, height=8)) == 0
    assert fwd(view=_lib.View(P=0, width=0, height=0)) == 0
    assert bwd(view=_lib.View(P=-1, width=8, height=8)) == INV
    # the forward's state and the required pointers, before any use
    assert fwd(geom_buffer=None) == INV and b"scratch buffers" in L.lr_last_error()
    assert fwd(out_features=None) == INV and b"required" in L.lr_last_error()
    assert fwd(features=None) == INV and b"required" in L.lr_last_error()
    assert bwd(geom_buffer=None) == INV and b"scratch buffers" in L.lr_last_error()
    for missing in ("features", "dL_dout_features", "out_features", "dL_dfeatures", "workspace", "dL_dmean2D", "dL_dopacity",
                    "dL_dmean3D", "dL_dscale", "dL_drot"):
        assert bwd(**{missing: None}) == INV, missing
        assert b"required" in L.lr_last_error(), missing
    v = _lib.View(P=5, width=8, height=8, means3D=64, viewmatrix=64, projmatrix=64, cov3D_precomp=64)
    assert bwd(view=v) == INV and b"dL_dcov3D" in L.lr_last_error()
    v = _lib.View(P=5, width=8, height=8, means3D=64, viewmatrix=64, projmatrix=64)
    assert bwd(view=v) == INV and b"scales+rotations or cov3D_precomp" in L.lr_last_error()
    # alignment
    assert fwd(features=68) == INV and b"16-byte" in L.lr_last_error()
    assert fwd(out_features=72) == INV and b"16-byte" in L.lr_last_error()
    for name in ("features", "dL_dfeatures", "workspace", "dL_dmean3D"):
        assert bwd(**{name: 68}) == INV, name
        assert b"16-byte" in L.lr_last_error(), name
    # a short workspace (async mode: the capacity bounds the slots)
    need = L.lr_features_workspace_bytes(100, 8)
    assert bwd(workspace_bytes=need - 1) == INV and b"workspace_bytes" in L.lr_last_error()
    assert bwd(workspace_bytes=0, binning_capacity=0) == INV and b"workspace_bytes" in L.lr_last_error()


def test_workspace_bytes_is_monotone_and_zero_for_invalid_arguments():
    from luciddreamer_amd import _lib, build
    build.build()
    wb = _lib.lib().lr_features_workspace_bytes
    assert wb(-1, 8) == 0 and wb(10, 0) == 0 and wb(10, -3) == 0 and wb(10, _lib.LR_FEATURE_MAX_CHANNELS + 1) == 0
    slots = [0, 1, 2, 63, 64, 1000, 12345, 1 << 20, (1 << 31) + 5]
    chans = [1, 3, fr.K - 1, fr.K, fr.K + 1, 2 * fr.K + 1, _lib.LR_FEATURE_MAX_CHANNELS]
    table = [[wb(s, c) for c in chans] for s in slots]
    for i, row in enumerate(table):
        assert all(b > 0 for b in row) and all(x <= y for x, y in zip(row, row[1:])), row
        if i:
            assert all(x <= y for x, y in zip(table[i - 1], row))
    assert wb((1 << 31) + 5, 8) >= ((1 << 31) + 5) * 4 * fr.K and wb(1000, 8) >= 1000 * 4 * fr.K


def test_python_refuses_a_wrong_table_before_any_launch():
    """ValueError from the wrappers and the operators without a device: nothing has been launched when it is raised."""
    from luciddreamer_amd import _C
    from luciddreamer_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians, rasterize_gaussians_raw
    P = 4
    empty = torch.Tensor([])
    rs = GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    bad = {"a (P, C) tensor": torch.zeros(P), "float32": torch.zeros(P, 5, dtype=torch.float64), "rows": torch.zeros(P + 1, 5),
           "channels": torch.zeros(P, _C.FEATURE_MAX_CHANNELS + 1)}
    for what, f in bad.items():
        with pytest.raises(ValueError, match=re.escape(what)):
            rasterize_gaussians(torch.zeros(P, 3), torch.zeros(P, 3), empty, torch.zeros(P, 3), torch.zeros(P, 1), torch.ones(P, 3),
                                torch.ones(P, 4), empty, rs, features=f)
        with pytest.raises(ValueError, match=re.escape(what)):
            GaussianRasterizer(rs)(torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 1), colors_precomp=torch.zeros(P, 3),
                                   scales=torch.ones(P, 3), rotations=torch.ones(P, 4), features=f)
        with pytest.raises(ValueError, match=re.escape(what)):
            rasterize_gaussians_raw(torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 1, 3), torch.zeros(P, 0, 3), torch.zeros(P, 1),
                                    torch.zeros(P, 3), torch.ones(P, 4), rs, features=f)
        with pytest.raises(ValueError, match=re.escape(what)):
            _C.render_features_backward(empty, empty, empty, empty, empty, f, torch.zeros(P, dtype=torch.int32), rs,
                                        means3D=torch.zeros(P, 3), slots=1)
        if what != "rows":
            with pytest.raises(ValueError, match=re.escape(what)):
                _C.render_features(empty, empty, empty, f, rs)
    with pytest.raises(ValueError, match="channels"):
        _C.render_features(empty, empty, empty, torch.zeros(P, 0), rs)
