"""The 3D smoothing filter on the device (csrc/filter3d.hip through luciddreamer_amd.filter3d) against the float64 NumPy
reference of tests/filter3d_ref.py, on the cases of tests/filter3d_cases.py.

Tolerances are not chosen, they are measured per case, the way tests/test_gpu_mcmc.py takes them: the same inputs go through
the float32 restatement of the kernel's operations on the CPU, its largest distance from the float64 reference is what float32
arithmetic costs on those inputs, and the device may be FOUR times as far -- the margin for expf / logf / log1pf / expm1f
differing by a few ulp between the host's and the device's.  Every test prints the measured value, the bar and the device's
distance before it asserts.  Distances are max |value - reference| over a tensor.  What is said to be exact is compared bit for bit.
"""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import filter3d_cases as C
from tests import filter3d_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev_update(xyz, cams, dev, variance=0.2):
    from luciddreamer_amd import filter3d
    f, seen = filter3d.compute_filter_3d(torch.from_numpy(xyz).to(dev), torch.from_numpy(cams).to(dev), variance, return_seen=True)
    assert f.shape == (xyz.shape[0], 1) and f.dtype == torch.float32 and seen.dtype == torch.bool
    return f.cpu().numpy()[:, 0], seen.cpu().numpy()


# ---- update ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_update_against_the_reference(hip_device, name):
    """Recorded on an MI355X with this file: the restatement's distance is 2.2e-09 .. 5.5e-09 over the seeded cases that see
    something (9.3e-10 hand-placed, 8.5e-10 mixed-focal), the bars four times that, and the device's distance equals the
    restatement's in every case, because its filter has the restatement's BITS: every operation of k_filter3d_rate is a single
    correctly rounded float32 operation (the file is compiled without FMA contraction) in the order the restatement uses.  That
    is asserted too: it is what keeps a visibility test from being decided differently on the device."""
    xyz, cams = C.all_cases()[name]
    f64, seen64 = R.update(xyz, cams)
    f32, _ = R.update(xyz, cams, dtype=np.float32)
    e32 = float(np.abs(f32.astype(np.float64) - f64).max())
    got, seen = dev_update(xyz, cams, hip_device)
    err = float(np.abs(got.astype(np.float64) - f64).max())
    print(f"update {name}: float32 restatement {e32:.3e}  bar {4 * e32:.3e}  device {err:.3e}  seen {int(seen.sum())}/{len(seen)}"
          f"  bit-equal to the restatement: {np.array_equal(bits(got), bits(f32))}")
    assert np.array_equal(seen, seen64)                                       # exact: no case has a fragile pair
    assert err <= 4 * e32, (err, e32)
    assert np.array_equal(bits(got), bits(f32))
    if seen.any():
        assert np.all(bits(got[~seen]) == bits(got[seen].max()))              # the widest filter in use, to the bit
        assert got[seen].min() > 0
    else:
        assert not bits(got).any()                                            # +0.0 everywhere
    again, seen_again = dev_update(xyz, cams, hip_device)
    assert np.array_equal(bits(again), bits(got)) and np.array_equal(seen_again, seen)
    # without the seen output: the same filter
    from luciddreamer_amd import filter3d
    alone = filter3d.compute_filter_3d(torch.from_numpy(xyz).to(hip_device), torch.from_numpy(cams).to(hip_device))
    assert np.array_equal(bits(alone.cpu().numpy()[:, 0]), bits(got))


def test_update_hand_placed_rows(hip_device):
    xyz, cams = C.hand_placed()
    got, seen = dev_update(xyz, cams, hip_device)
    assert tuple(bool(s) for s in seen) == C.HAND_SEEN
    want = math.sqrt(0.2) * 3.0 / float(cams[0, 16])                          # the on-axis row at depth 3
    assert abs(got[-1] - want) <= 2e-7 * want and np.all(bits(got[~seen]) == bits(got[-1]))


def test_update_mixed_focal_lengths_follow_the_paper(hip_device):
    xyz, cams = C.mixed_focal()
    got, seen = dev_update(xyz, cams, hip_device)
    sv, fa, fb = math.sqrt(0.2), float(cams[0, 16]), float(cams[1, 16])
    assert list(seen) == [True, True, False]
    assert abs(got[0] - sv * 4.0 / fb) <= 1e-6 * got[0]                       # min z / fx; min z / max fx would be half of it
    assert abs(got[1] - sv * 2.0 / fa) <= 1e-6 * got[1] and bits(got[2]) == bits(got[1])


@pytest.mark.parametrize("P", [1, 65, 1037])
def test_update_without_cameras_or_without_anything_seen_gives_zeros(hip_device, P):
    xyz = C.seeded(P, 3)[0]
    got, seen = dev_update(xyz, np.zeros((0, 20), np.float32), hip_device)
    assert not seen.any() and not bits(got).any()
    behind = xyz.copy()
    behind[:, 2] = -1.0 - np.abs(behind[:, 2])
    got, seen = dev_update(behind, C.path(3), hip_device)
    assert not seen.any() and not bits(got).any()


def test_update_takes_camera_objects_and_a_variance(hip_device):
    from luciddreamer_amd import cameras, filter3d
    xyz, packed = C.seeded(257, 3)
    cams = [c.to(hip_device) for c in cameras.lookaround_path(C.W, C.H, n_views=3)]
    x = torch.from_numpy(xyz).to(hip_device)
    a = filter3d.compute_filter_3d(x, cams)
    b = filter3d.compute_filter_3d(x, torch.from_numpy(packed).to(hip_device))
    assert torch.equal(a, b)
    c = filter3d.compute_filter_3d(x, cams, variance=0.8)
    assert torch.allclose(c, 2 * a, rtol=1e-6, atol=0)
    assert filter3d.compute_filter_3d(x[:0], cams).shape == (0, 1)
    with pytest.raises(ValueError, match="variance"):
        filter3d.compute_filter_3d(x, cams, variance=-1.0)


# ---- apply ----------------------------------------------------------------------------------------------------------------
def dev_apply(r, q, f, activated, dev, g=None, go=None, needs=(True, True)):
    """(scale out, opacity out, dL/dr, dL/dq) through the autograd function; upstreams None = that output is not used."""
    from luciddreamer_amd import filter3d
    rt = torch.from_numpy(r).to(dev).requires_grad_(True)
    qt = torch.from_numpy(q).to(dev).requires_grad_(True)
    s, o = filter3d.apply(rt, qt, torch.from_numpy(f).to(dev), activated=activated)
    assert s.shape == rt.shape and o.shape == qt.shape
    outs, ups = [], []
    if g is not None:
        outs.append(s), ups.append(torch.from_numpy(g).to(dev))
    if go is not None:
        outs.append(o), ups.append(torch.from_numpy(go).to(dev))
    dr = dq = None
    if outs:
        torch.autograd.backward(outs, ups)
        dr, dq = rt.grad.cpu().numpy(), qt.grad.cpu().numpy()[:, 0]
    return s.detach().cpu().numpy(), o.detach().cpu().numpy()[:, 0], dr, dq


@pytest.mark.parametrize("activated", [False, True], ids=["stored", "activated"])
@pytest.mark.parametrize("P", C.P_VALUES)
def test_apply_forward_and_backward_against_the_reference(hip_device, P, activated):
    """r in [-12, 2], q in [-12, 12], f in {0} U [1e-4, 1].  Recorded on an MI355X with this file (float32 restatement on the
    CPU / bar = 4 x / device), the two ends of the sizes:
        stored    P = 1     scale 9.64e-08 / 3.86e-07 / 9.64e-08      opacity 1.68e-07 / 6.73e-07 / 1.68e-07
                            dL/dscale 3.48e-08 / 1.39e-07 / 2.48e-08  dL/dopacity 5.20e-09 / 2.08e-08 / 5.20e-09
        activated P = 1     scale 7.23e-09 / 2.89e-08 / 7.23e-09      opacity 2.84e-13 / 1.14e-12 / 3.98e-13
                            dL/dscale 6.95e-11 / 2.78e-10 / 6.96e-11  dL/dopacity 1.66e-13 / 6.63e-13 / 2.23e-13
        stored    P = 1037  scale 9.13e-07 / 3.65e-06 / 1.27e-06      opacity 2.39e-06 / 9.56e-06 / 2.39e-06
                            dL/dscale 1.10e-06 / 4.40e-06 / 1.96e-06  dL/dopacity 1.75e-07 / 6.98e-07 / 1.75e-07
        activated P = 1037  scale 8.05e-07 / 3.22e-06 / 7.35e-07      opacity 2.65e-07 / 1.06e-06 / 2.65e-07
                            dL/dscale 2.09e-06 / 8.36e-06 / 2.09e-06  dL/dopacity 1.87e-07 / 7.49e-07 / 1.39e-07
    Over all twelve cases the device is at most 1.9 x the restatement's distance (stored scale, P = 257); the largest stored
    logit error is 3.3e-06 (P = 65).  The single row of P = 1 is a filtered one: see filter3d_cases.apply_inputs."""
    r, q, f, g, go = C.apply_inputs(P)
    s64, o64 = R.apply64(r, q, f, activated)
    s32, o32 = R.apply32(r, q, f, activated)
    dr64, dq64 = R.backward64(r, q, f, g, go, activated)
    dr32, dq32 = R.backward32(r, q, f, g, go, activated)
    s, o, dr, dq = dev_apply(r, q, f, activated, hip_device, g, go)
    dist = lambda a, b: float(np.abs(a.astype(np.float64) - b).max())
    rows = (("scale", s, s32, s64), ("opacity", o, o32, o64), ("dL/dscale", dr, dr32, dr64), ("dL/dopacity", dq, dq32, dq64))
    domain = "activated" if activated else "stored"
    for what, got, f32, f64 in rows:
        print(f"apply {domain} P={P} {what}: float32 restatement {dist(f32, f64):.3e}  bar {4 * dist(f32, f64):.3e}  "
              f"device {dist(got, f64):.3e}")
    for what, got, f32, f64 in rows:
        assert np.isfinite(got).all(), what
        assert dist(got, f64) <= 4 * dist(f32, f64), (what, dist(got, f64), dist(f32, f64))
    off = f[:, 0] == 0
    if not activated:                                                          # no filter: the stored domain keeps its bits
        assert np.array_equal(bits(s[off]), bits(r[off])) and np.array_equal(bits(o[off]), bits(q[off, 0]))
        assert np.array_equal(bits(dr[off]), bits(g[off])) and np.array_equal(bits(dq[off]), bits(go[off, 0]))
    if P > 1:
        assert off.any() and not off.all()
    # bit-repeatable
    s2, o2, dr2, dq2 = dev_apply(r, q, f, activated, hip_device, g, go)
    for a, b in ((s, s2), (o, o2), (dr, dr2), (dq, dq2)):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("activated", [False, True], ids=["stored", "activated"])
def test_apply_extreme_row_is_finite(hip_device, activated):
    """r = -40, f = 1, q = 3: t = exp(80), the branch for t > 1.  s' = f and o' = sigmoid(3) exp(-120) to float32."""
    r, q, f = np.full((1, 3), -40, np.float32), np.full((1, 1), 3, np.float32), np.ones((1, 1), np.float32)
    g, go = np.ones((1, 3), np.float32), np.ones((1, 1), np.float32)
    s, o, dr, dq = dev_apply(r, q, f, activated, hip_device, g, go)
    for a in (s, o, dr, dq):
        assert np.isfinite(a).all()
    if activated:
        assert np.allclose(s, 1.0, rtol=1e-6) and o[0] >= 0 and o[0] < 1e-37
    else:
        assert np.allclose(s, 0.0, atol=1e-6) and abs(o[0] - (math.log(1 / (1 + math.exp(-3.0))) - 120.0)) < 1e-4


@pytest.mark.parametrize("activated", [False, True], ids=["stored", "activated"])
@pytest.mark.parametrize("P", [65, 1037])
def test_apply_null_upstream_is_a_zero_upstream(hip_device, P, activated):
    """An output nobody used reaches the kernel as NULL; the gradients are those of an explicit zero tensor, to the bit."""
    from luciddreamer_amd import filter3d
    r, q, f, g, go = C.apply_inputs(P)
    t = lambda a: torch.from_numpy(a).to(hip_device)
    _, _, dr_a, dq_a = dev_apply(r, q, f, activated, hip_device, g, None)                 # through autograd: opacity output unused
    dr_b, dq_b = filter3d.backward(t(r), t(q), t(f), t(g), torch.zeros_like(t(go)), activated=activated)
    assert np.array_equal(bits(dr_a), bits(dr_b.cpu().numpy())) and np.array_equal(bits(dq_a), bits(dq_b.cpu().numpy()[:, 0]))
    _, _, dr_a, dq_a = dev_apply(r, q, f, activated, hip_device, None, go)                # scale output unused
    dr_b, dq_b = filter3d.backward(t(r), t(q), t(f), torch.zeros_like(t(g)), t(go), activated=activated)
    assert np.array_equal(bits(dr_a), bits(dr_b.cpu().numpy())) and np.array_equal(bits(dq_a), bits(dq_b.cpu().numpy()[:, 0]))
    dr_n, dq_n = filter3d.backward(t(r), t(q), t(f), None, None, activated=activated)
    assert not dr_n.any() and not dq_n.any()


def test_apply_refuses_a_filter_of_another_length(hip_device):
    from luciddreamer_amd import filter3d
    r, q, f, _, _ = C.apply_inputs(65)
    t = lambda a: torch.from_numpy(a).to(hip_device)
    with pytest.raises(ValueError, match="recompute"):
        filter3d.apply(t(r), t(q), t(f)[:64])
    s, o = filter3d.apply(t(r), t(q), t(f)[:, 0])                                          # [P] is as good as [P,1]
    s2, o2 = filter3d.apply(t(r), t(q), t(f))
    assert torch.equal(s, s2) and torch.equal(o, o2)
    with pytest.raises(RuntimeError, match="HIP device"):
        filter3d.apply(t(r), t(q), torch.from_numpy(f))


# ---- through the unchanged paths -----------------------------------------------------------------------------------------
W = H = 64
P_INT = 257


@pytest.fixture(scope="module")
def scene(hip_device):
    """A 257-Gaussian box cloud at 64x64 under the identity camera, its filter from a 3-view path and the identity camera, the
    stored-domain values baked into a plain cloud, and one upstream image gradient."""
    from luciddreamer_amd import cameras, filter3d, synthetic
    from luciddreamer_amd.gaussian_renderer import GaussianCloud
    cloud = {k: v.to(hip_device) for k, v in synthetic.make_cloud(P_INT, "box", 3).items()}
    mk = lambda: GaussianCloud(cloud["means3D"], cloud["scales"], cloud["rotations"], cloud["opacities"], cloud["shs"])
    m = mk()
    cam = cameras.identity_camera(W, H).to(hip_device)
    f = filter3d.compute_filter_3d(m._xyz.detach(), [cam] + [c.to(hip_device) for c in cameras.lookaround_path(W, H, n_views=3)])
    assert bool((f > 0).all())
    with torch.no_grad():
        bs, bo = filter3d.apply(m._scaling, m._opacity, f)
    plain = mk()
    plain._scaling = bs.clone().requires_grad_(True)
    plain._opacity = bo.clone().requires_grad_(True)
    return dict(m=m, plain=plain, cam=cam, f=f, baked=(bs, bo), gcol=synthetic.upstream_grad(H, W, seed=3).to(hip_device))


def test_render_raw_of_the_view_is_render_raw_of_the_baked_cloud(hip_device, scene):
    from luciddreamer_amd import filter3d
    from luciddreamer_amd.gaussian_renderer import render, render_raw
    m, plain, cam, f = scene["m"], scene["plain"], scene["cam"], scene["f"]
    for p in m.parameters() + plain.parameters() + [plain._scaling, plain._opacity]:
        p.grad = None
    view = filter3d.filtered(m, f)
    out_v = render_raw(cam, view)
    out_p = render_raw(cam, plain)
    assert torch.equal(out_v["render"], out_p["render"]) and torch.equal(out_v["radii"], out_p["radii"])
    assert float(out_v["render"].detach().abs().max()) > 0
    assert not torch.equal(out_v["render"], render_raw(cam, m, render_only=True)["render"])     # the filter does something
    (out_v["render"] * scene["gcol"]).sum().backward()
    (out_p["render"] * scene["gcol"]).sum().backward()
    # the view's gradients on the model's own parameters: the filter's backward of the plain cloud's gradients, to the bit
    want_s, want_o = filter3d.backward(m._scaling, m._opacity, f, plain._scaling.grad, plain._opacity.grad, activated=False)
    assert torch.equal(m._scaling.grad, want_s) and torch.equal(m._opacity.grad, want_o)
    assert float(m._scaling.grad.abs().max()) > 0 and float(m._opacity.grad.abs().max()) > 0
    for a in ("_xyz", "_rotation", "_features_dc", "_features_rest"):                           # forwarded, not copied
        assert torch.equal(getattr(m, a).grad, getattr(plain, a).grad), a
    # each pair is computed once per view, and everything else is the model's
    assert view._scaling is view._scaling and view._opacity is view._opacity and view.get_scaling is view.get_scaling
    assert view._xyz is m._xyz and view.get_xyz is m.get_xyz and view.active_sh_degree == m.active_sh_degree
    assert view.max_sh_degree == m.max_sh_degree and view._features_rest is m._features_rest
    assert torch.equal(view.get_rotation, m.get_rotation) and torch.equal(view.get_features, m.get_features)
    # the activated getters feed render(): the same picture up to the rounding of the activations
    again = filter3d.filtered(m, f)
    out_a = render(cam, again)
    assert float((out_a["render"] - out_v["render"]).abs().max()) <= 2e-5
    assert torch.allclose(again.get_scaling, torch.exp(scene["baked"][0]), rtol=1e-5, atol=0)
    with pytest.raises(AttributeError, match="read-only"):
        view.active_sh_degree = 0


def test_save_ply_of_the_view_writes_the_baked_values(hip_device, scene, tmp_path):
    from luciddreamer_amd import densify, filter3d
    m, f = scene["m"], scene["f"]
    bs, bo = scene["baked"]
    path = str(tmp_path / "fused.ply")
    densify.save_ply(filter3d.filtered(m, f), path)
    v = densify.read_ply(path)
    assert np.array_equal(bits(v["opacity"]), bits(bo.cpu().numpy()[:, 0]))
    for j in range(3):
        assert np.array_equal(bits(v[f"scale_{j}"]), bits(bs.cpu().numpy()[:, j]))
    assert np.array_equal(bits(v["x"]), bits(m._xyz.detach().cpu().numpy()[:, 0]))
    assert not np.array_equal(v["opacity"], m._opacity.detach().cpu().numpy()[:, 0])


def _example():
    spec = importlib.util.spec_from_file_location("train_loop_example_filter3d_gpu", os.path.join(ROOT, "examples", "train_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("multi_view", [0, 2])
def test_example_loop_with_the_filter(hip_device, multi_view):
    mod = _example()
    losses, _ = mod.train(mod.default_args(gaussians=2000, iters=30, resolution="64x64", filter3d=True, multi_view=multi_view),
                          log=lambda s: None)
    assert losses and all(math.isfinite(l) for _, l, _ in losses)


@pytest.mark.parametrize("multi_view", [0, 2])
def test_filter_length_follows_the_set_across_a_densification(hip_device, multi_view, monkeypatch):
    from luciddreamer_amd import filter3d
    mod = _example()
    lengths = []
    real = filter3d.compute_filter_3d

    def recording(xyz, *a, **kw):
        out = real(xyz, *a, **kw)
        lengths.append(int(out.shape[0]))
        return out
    monkeypatch.setattr(filter3d, "compute_filter_3d", recording)
    losses, _ = mod.train(mod.default_args(gaussians=2000, iters=30, resolution="64x64", filter3d=True, multi_view=multi_view,
                                           densify_from=10, densify_every=10, densify_grad_threshold=1e-6, log=1),
                          log=lambda s: None)
    assert all(math.isfinite(l) for _, l, _ in losses)
    counts = [p for _, _, p in losses]
    assert len(set(counts)) > 1, "densify_and_prune never changed the number of Gaussians"
    # after build and after the densifications of iterations 10, 20 and 30 (the threshold is low enough for every one to act)
    assert lengths == [1000, counts[9], counts[19], counts[29]]
