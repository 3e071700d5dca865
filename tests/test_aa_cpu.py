"""Anti-aliasing (config.set_antialiasing, lr_set_antialiasing) without a GPU: the algebra of the backward against float64
autograd, the float32 restatement of the coefficient against float64 on the inputs the GPU tests use, the C-ABI and the
kernel symbols of the built library, and the Python switch."""
import os
import struct

import numpy as np
import pytest
import torch

from tests import aa_cases, aa_ref


def _leaves(cloud, cov=False):
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    d = dict(means3D=leaf(cloud["means3D"]))
    if cov:
        d["cov3D"] = leaf(aa_ref.cov3d64(cloud["scales"].double(), cloud["rotations"].double()))
    else:
        d["scales"], d["rotations"] = leaf(cloud["scales"]), leaf(cloud["rotations"])
    return d


@pytest.mark.parametrize("case", [0, 1])
@pytest.mark.parametrize("cov", [False, True], ids=["scale_rot", "cov3D"])
def test_closed_form_backward_equals_autograd(case, cov):
    """dL/dopacity = g coef and the three covariance terms of the issue (aa_ref.closed_form_cov_grads, what
    csrc/gauss_bwd.hip adds to dL_da / dL_db / dL_dc), carried on by autograd of the covariance chain, against autograd of
    L = sum g_i opacity_i coef64_i -- float64 against float64, 1e-8 of each tensor's maximum.  The clouds hold sub-pixel,
    needle-shaped and clamped Gaussians and Gaussians beyond the 1.3 tan_fov clamp."""
    cam, cloud = aa_cases.grad_case(case, outside_clamp=True)
    tfx, tfy = aa_cases.tan_fov(cam)
    W, H = cam.image_width, cam.image_height
    V = cam.world_view_transform
    gen = torch.Generator().manual_seed(77 + case)
    P = cloud["means3D"].shape[0]
    g = torch.randn(P, generator=gen, dtype=torch.float64)
    op = cloud["opacities"][:, 0].double().clone().requires_grad_(True)
    kw = lambda d: dict(cov3D_precomp=d["cov3D"]) if cov else dict(scales=d["scales"], rotations=d["rotations"])

    a = _leaves(cloud, cov)
    full = aa_ref.coef64(a["means3D"], V, tfx, tfy, W, H, full=True, **kw(a))
    front = full["vz"].detach() > 0.2
    assert int(front.sum()) > 0.9 * P
    rho = full["rho"].detach()
    n_clamped = int(((rho <= aa_ref.RHO_FLOOR) & front).sum())
    txtz = (a["means3D"].detach() @ V.double()[:3, :3] + V.double()[3, :3])
    n_outside = int((((txtz[:, 0] / txtz[:, 2]).abs() > 1.3 * tfx) & front).sum())
    assert n_clamped >= aa_cases.N_SPECIAL and n_outside >= aa_cases.N_SPECIAL // 2, (n_clamped, n_outside)
    assert int(((rho > aa_ref.RHO_FLOOR) & (rho < 0.05) & front).sum()) >= aa_cases.N_SPECIAL // 2      # sub-pixel / needles
    (g * op * full["coef"]).sum().backward()
    want = {k: v.grad.clone() for k, v in a.items()}
    want["opacity"] = op.grad.clone()

    b = _leaves(cloud, cov)
    a0, bb, c0, vz = aa_ref.cov2d64(b["means3D"], V, tfx, tfy, W, H, **kw(b))
    coef = aa_ref.coef_from_cov64(a0.detach(), bb.detach(), c0.detach())[0]
    coef = torch.where(vz.detach() > 0.2, coef, torch.ones_like(coef))
    rec_op = op.detach() * coef                              # what the kernel reads back from the record
    g_front = torch.where(vz.detach() > 0.2, g, torch.zeros_like(g))          # preprocess projects nothing behind the near plane
    da0, db, dc0 = aa_ref.closed_form_cov_grads(g_front, rec_op, a0.detach(), bb.detach(), c0.detach())
    torch.autograd.backward([a0, bb, c0], [da0, db, dc0])
    got = {k: v.grad for k, v in b.items()}
    got["opacity"] = g * coef
    for k in want:
        scale = float(want[k].abs().max())
        err = float((got[k] - want[k]).abs().max())
        print(f"{k}: max|closed form - autograd| = {err:.3e}, max|autograd| = {scale:.3e}")
        assert scale > 0 and err <= 1e-8 * scale, (k, err, scale)
    # clamped Gaussians: the coefficient is a constant, no geometry gradient at all
    cl = (rho <= aa_ref.RHO_FLOOR) & front
    for k in a:
        assert not bool(want[k][cl].any()) and not bool(got[k][cl].any()), k


def _gpu_inputs():
    """(name, cam, cloud, kwargs of coef32/coef64) of every view the GPU gradient tests differentiate."""
    for i in range(len(aa_cases.GRAD_CASES)):
        cam, cloud = aa_cases.grad_case(i)
        yield f"grad{i}", cam, cloud
    for i in range(len(aa_cases.FORWARD_CASES)):
        cam, cloud = aa_cases.box_case(*aa_cases.FORWARD_CASES[i])
        yield f"forward{i}", cam, cloud


def test_coef32_against_coef64_on_the_gpu_test_inputs():
    """det0 = a0 c0 - b b cancels for thin splats, so the float32 coefficient the kernels produce can be far from the float64
    one; the GPU gradient test composes its expectation from both and must only see inputs where they agree.  Reports the
    worst relative error per input and where it occurs; the gradient inputs must stay within 1e-5 on every Gaussian the view
    renders (so that a GPU failure there means the kernel)."""
    from tests import helpers as hp
    for name, cam, cloud in _gpu_inputs():
        tfx, tfy = aa_cases.tan_fov(cam)
        W, H = cam.image_width, cam.image_height
        c32 = aa_cases.coef_of(cam, cloud, full=True)
        c64 = aa_ref.coef64(cloud["means3D"], cam.world_view_transform, tfx, tfy, W, H, cloud["scales"], cloud["rotations"],
                            full=True)
        radii = hp.run_oracle(cloud, cam, 0, torch.zeros(3), use_sh=True)["radii"]
        vis = radii > 0
        rel = np.abs(c32["coef"].astype(np.float64) - c64["coef"].numpy()) / c64["coef"].numpy()
        rel_vis = np.where(vis, rel, 0.0)
        w = int(rel_vis.argmax())
        print(f"{name}: {int(vis.sum())} visible of {vis.size}; worst relative error of coef32 {rel_vis[w]:.3e} at Gaussian {w} "
              f"(rho {float(c64['rho'][w]):.3e}, det0 {float(c64['det0'][w]):.3e}, a0 {float(c64['a0'][w]):.3e}, "
              f"c0 {float(c64['c0'][w]):.3e}, b {float(c64['b'][w]):.3e}); clamped and visible: "
              f"{int((vis & (c32['rho'] <= np.float32(aa_ref.RHO_FLOOR))).sum())}")
        if name.startswith("grad"):
            assert rel_vis[w] <= 1e-5, (name, w, rel_vis[w])
            # both sides agree on which Gaussians are clamped (the branch has a zero geometry gradient)
            assert np.array_equal((c32["rho"] <= np.float32(aa_ref.RHO_FLOOR))[vis], (c64["rho"].numpy() <= aa_ref.RHO_FLOOR)[vis])
            assert int((vis & (c32["rho"] <= np.float32(aa_ref.RHO_FLOOR))).sum()) >= 4


def test_coef32_restates_the_projection_of_the_oracle_bit_for_bit():
    """The float32 chain of aa_ref (view transform, 3D covariance, Jacobian, EWA product) gives the conic the C oracle -- and
    with it the kernels -- computes, bit for bit: the coefficient is formed from the very a0, b, c0 of preprocess."""
    from tests import helpers as hp
    for cam, cloud, sm in [aa_cases.box_case(*aa_cases.FORWARD_CASES[1]) + (1.0,), aa_cases.grad_case(0) + (1.7,)]:
        ref = hp.run_oracle(cloud, cam, 0, torch.zeros(3), scale_modifier=sm)
        o = aa_cases.coef_of(cam, cloud, scale_modifier=sm, full=True)
        vis = ref["radii"] > 0
        det_inv = np.float32(1.0) / o["det"]
        conic = np.stack([o["c"] * det_inv, -o["b"] * det_inv, o["a"] * det_inv], 1).astype(np.float32)
        assert np.array_equal(conic[vis].view(np.uint32), ref["res"].stage()["conic_opacity"][vis, :3].view(np.uint32))


def test_prescaled_oracle_inputs_stay_inside_the_fragile_pixel_cap():
    """The GPU forward test feeds the oracle `opacity * coef32`; helpers.compare_forward caps the pixels the oracle flags as
    sitting on a threshold at max(8, 2e-4 pixels).  Checked here, before any GPU time is spent."""
    from tests import helpers as hp
    for name, cam, cloud in _gpu_inputs():
        ref = hp.run_oracle(aa_cases.prescaled(cloud, aa_cases.coef_of(cam, cloud)), cam, 0, torch.zeros(3))
        frag = int(((ref["res"].stage()["fragile"] & 1) != 0).sum())
        cap = max(8, hp.FRAGILE_FRAC * cam.image_width * cam.image_height)
        print(f"{name}: {frag} flagged pixels (cap {cap})")
        assert frag <= cap, (name, frag, cap)


# ---- the built library and the Python switch (these fail without the feature) ------------------------------------------------
def _gfx950_code_objects(path):
    data = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, pos = [], 0
    while True:
        i = data.find(magic, pos)
        if i < 0:
            return out
        pos = i + 1
        n = struct.unpack_from("<Q", data, i + 24)[0]
        p = i + 32
        if n > 16:
            continue
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tl]
            p += tl
            if b"gfx950" in triple and size:
                out.append(data[i + off:i + off + size])


def test_library_exports_the_setting_and_round_trips():
    from luciddreamer_amd import _lib
    L = _lib.lib()
    assert "lr_set_antialiasing" in _lib.EXPORTS and "lr_get_antialiasing" in _lib.EXPORTS
    L.lr_set_antialiasing(0)
    try:
        assert L.lr_get_antialiasing() == 0
        assert L.lr_set_antialiasing(1) == 0 and L.lr_get_antialiasing() == 1          # returns the previous value
        assert L.lr_set_antialiasing(7) == 1 and L.lr_get_antialiasing() == 1
        assert L.lr_set_antialiasing(0) == 1 and L.lr_get_antialiasing() == 0
    finally:
        L.lr_set_antialiasing(0)
    assert b" 0.6" in L.lr_version()
    with pytest.raises(RuntimeError):
        _lib.tune_set("antialiasing", 1)              # not a tuning knob: it changes results


def test_code_object_holds_the_antialiased_kernels():
    from luciddreamer_amd import build
    assert os.path.exists(build.LIB_PATH)
    blob = b"".join(_gfx950_code_objects(build.LIB_PATH))
    assert blob, "no gfx950 code object in the library"
    # Itanium mangling of k<RAW, AA>: I Lb<RAW>E Lb<AA>E E
    for kernel in (b"12k_preprocess", b"17k_preprocess_pool", b"11k_gauss_bwd", b"17k_gauss_bwd_depth"):
        for raw in (b"0", b"1"):
            for aa in (b"0", b"1"):
                sym = kernel + b"ILb" + raw + b"ELb" + aa + b"EE"
                assert sym in blob, sym.decode()


def test_config_switch_defaults_off_and_reset_clears_it():
    from luciddreamer_amd import _lib, config
    _lib.lib().lr_set_antialiasing(0)
    assert config.antialiasing() is False
    try:
        config.set_antialiasing(True)
        assert config.antialiasing() is True and _lib.lib().lr_get_antialiasing() == 1
        config.require_antialiasing(True)
        with pytest.raises(RuntimeError, match="anti-aliasing"):
            config.require_antialiasing(False)
        config.reset()
        assert config.antialiasing() is False and _lib.lib().lr_get_antialiasing() == 0
        config.set_antialiasing(True)
        config.set_antialiasing(False)
        assert config.antialiasing() is False
    finally:
        config.set_antialiasing(False)


def test_settings_keep_their_twelve_fields():
    from depth_diff_gaussian_rasterization_min import GaussianRasterizationSettings
    assert len(GaussianRasterizationSettings._fields) == 12
