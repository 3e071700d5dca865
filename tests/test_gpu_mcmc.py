"""MCMC densification on the device (csrc/mcmc.hip through luciddreamer_amd.mcmc) against the float64 NumPy restatement of
tests/mcmc_ref.py.

Tolerances are not chosen, they are measured per case: the same inputs go through the float32 restatement of the same
operation order on the CPU (the relocation's double sum kept in float64, as the kernel keeps it), its largest distance from the
float64 reference is what float32 arithmetic costs on those inputs, and the device may be FOUR times as far -- the margin for
expf / log1pf / expm1f differing by a few ulp between the host libm and the device, and for FMA contraction.  Every test prints
the measured value, the bar and the device's distance before it asserts.  What row movement there is must be exact to the bit.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import mcmc_ref as R

pytestmark = pytest.mark.gpu
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
        "scaling": "_scaling", "rotation": "_rotation"}
GROUPS = tuple(ATTR)
MIN_OPACITY = 0.005
logit = lambda p: math.log(p / (1.0 - p))


def make_params(P, seed, n_rest=15):
    """Seeded raw parameters: xyz in [-1, 1]^3, log-scales in [-6, -1], unnormalised quaternions (row P // 2 of norm 1e-3),
    opacities spread over [0.001, 0.999] evenly in logit, i.e. with as many nearly transparent as nearly opaque rows."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    p = {"xyz": f(rng.uniform(-1, 1, (P, 3))), "f_dc": f(rng.normal(size=(P, 1, 3))), "f_rest": f(0.1 * rng.normal(size=(P, n_rest, 3))),
         "opacity": f(rng.uniform(logit(0.001), logit(0.999), (P, 1))), "scaling": f(rng.uniform(-6, -1, (P, 3))),
         "rotation": f(rng.normal(size=(P, 4)))}
    q = p["rotation"][P // 2]
    p["rotation"][P // 2] = q * np.float32(1e-3 / np.linalg.norm(q))
    return p


def make_moments(params, seed):
    rng = np.random.default_rng(seed + 1000)
    m = {}
    for g in GROUPS:
        m[g + ".exp_avg"] = rng.normal(size=params[g].shape).astype(np.float32)
        m[g + ".exp_avg_sq"] = (rng.uniform(size=params[g].shape) + 0.1).astype(np.float32)
    return m


def pairs_for(P, params):
    """Hand-built (dst, src).  P = 2 is one source and one dead row.  Otherwise: a source sampled 60 times (N clamps at 51), one
    with opacity 0.9990, one sampled once, one sampled 3 times, further sources sampled 1-12 times, and untouched rows.  P = 65
    has 65 rows: the 60 copies leave room for ONE more pair, so the opacity-0.9990 source is its sampled-once source and it has
    no source sampled 3 times (that case runs at 257 and 1037)."""
    rng = np.random.default_rng(P)
    rows = list(rng.permutation(P))
    take = lambda k: [int(rows.pop()) for _ in range(k)]
    if P == 2:
        s, = take(1)
        return np.array(take(1)), np.array([s])
    c60, d999 = take(2)
    params["opacity"][d999, 0] = np.float32(logit(0.9990))
    dst, src = [], []

    def add(s, k):
        k = min(k, len(rows) - 2)                                  # two rows at least stay untouched
        dst.extend(take(k))
        src.extend([s] * k)
    add(c60, 60)
    add(d999, 1 if P == 65 else 2)
    if P > 65:
        add(take(1)[0], 1)
        add(take(1)[0], 3)
        while len(rows) > P // 3:                                  # a third of the rows stays untouched
            add(take(1)[0], int(rng.integers(1, 13)))
    order = rng.permutation(len(dst))                               # the pairs of one source are not adjacent
    return np.array(dst)[order], np.array(src)[order]


def to_dev(d, dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in d.items()}


def run_relocate(params, moments, dst, src, dev, rows=None):
    from luciddreamer_amd import mcmc
    p = to_dev(params, dev)
    m = to_dev(moments, dev) if moments is not None else None
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)
    mcmc.relocate_rows(i32(dst), i32(src), p, {g: m[g + ".exp_avg"] for g in GROUPS} if m else None,
                       {g: m[g + ".exp_avg_sq"] for g in GROUPS} if m else None, rows=rows, min_opacity=MIN_OPACITY, n_max=51)
    torch.cuda.synchronize()
    back = lambda d: {k: v.cpu().numpy() for k, v in d.items()} if d is not None else None
    return back(p), back(m)


def bars(ref64, ref32, touched):
    """{opacity, scaling}: (float32 restatement's max distance from the reference over the touched rows, 4 x that)."""
    out = {}
    for k in ("opacity", "scaling"):
        e = float(np.abs(ref32[k][touched].astype(np.float64) - ref64[k][touched]).max())
        out[k] = (e, 4.0 * e)
    return out


@pytest.mark.parametrize("P", [2, 65, 257, 1037])
def test_relocate_against_the_reference(hip_device, P):
    """Distance = max |stored logit(o') or log(s') - float64 reference| over the touched rows.  Recorded on an MI355X with this
    file (float32 restatement on the CPU / bar = 4 x / device):
        P = 2     opacity 1.71e-07 / 6.83e-07 / 1.71e-07    scaling 1.60e-07 / 6.39e-07 / 3.98e-07
        P = 65    opacity 8.05e-06 / 3.22e-05 / 6.14e-06    scaling 3.80e-07 / 1.52e-06 / 5.94e-07
        P = 257   opacity 4.26e-06 / 1.70e-05 / 4.74e-06    scaling 4.46e-07 / 1.78e-06 / 5.56e-07
        P = 1037  opacity 1.52e-05 / 6.08e-05 / 1.49e-05    scaling 1.44e-06 / 5.77e-06 / 1.44e-06
    (the opacity figures are those of the nearly opaque sources: float32 sigmoid leaves 1 - o only four or five digits)."""
    params = make_params(P, seed=P)
    dst, src = pairs_for(P, params)
    moments = make_moments(params, seed=P)
    touched = np.unique(np.concatenate((dst, src)))
    untouched = np.setdiff1d(np.arange(P), touched)
    assert len(set(dst)) == len(dst) and not set(dst) & set(src) and (P == 2 or len(untouched) >= 2)
    if P > 2:
        assert np.bincount(src).max() == 60
    ref64, mom_ref = R.relocate(params, moments, dst, src, MIN_OPACITY, 51)
    ref32, _ = R.relocate(params, None, dst, src, MIN_OPACITY, 51, dtype=np.float32)
    bar = bars(ref64, ref32, touched)
    got, mom = run_relocate(params, moments, dst, src, hip_device)
    # rows that are neither source nor destination: all 18 tensors keep their bits
    for k in GROUPS:
        assert np.array_equal(got[k][untouched].view(np.uint32), params[k][untouched].view(np.uint32)), k
    for k in mom:
        assert np.array_equal(mom[k][untouched].view(np.uint32), moments[k][untouched].view(np.uint32)), k
        assert not mom[k][touched].any(), k                                        # exactly zero at sources and destinations
        assert np.array_equal(mom[k], mom_ref[k]), k
    # destinations are copies of their sources, which keep what is not opacity or scale
    for k in ("xyz", "f_dc", "f_rest", "rotation"):
        assert np.array_equal(got[k][dst].view(np.uint32), params[k][src].view(np.uint32)), k
        assert np.array_equal(got[k][src].view(np.uint32), params[k][src].view(np.uint32)), k
    for k in ("opacity", "scaling"):
        assert np.array_equal(got[k][dst].view(np.uint32), got[k][src].view(np.uint32)), k      # one result per source
        err = float(np.abs(got[k][touched].astype(np.float64) - ref64[k][touched]).max())
        print(f"relocate P={P} {k}: float32 restatement {bar[k][0]:.3e}  bar {bar[k][1]:.3e}  device {err:.3e}")
    for k in ("opacity", "scaling"):
        err = float(np.abs(got[k][touched].astype(np.float64) - ref64[k][touched]).max())
        assert err <= bar[k][1], (k, err, bar[k])
    # bit-repeatable, and the same parameters without optimizer state
    again, mom_again = run_relocate(params, moments, dst, src, hip_device)
    bare, _ = run_relocate(params, None, dst, src, hip_device)
    for k in GROUPS:
        assert np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)), k
        assert np.array_equal(bare[k].view(np.uint32), got[k].view(np.uint32)), k
    for k in mom:
        assert np.array_equal(mom_again[k].view(np.uint32), mom[k].view(np.uint32)), k


# ---- the strategy over a model -------------------------------------------------------------------------------------------
class Model:
    """The attributes of a GaussianModel that the strategy touches, with one optimizer step behind it."""

    def __init__(self, P, dev, seed, optimizer="fused", with_state=True):
        from luciddreamer_amd.optim import FusedAdam
        self.np_params = make_params(P, seed)
        for g, a in ATTR.items():
            setattr(self, a, nn.Parameter(torch.from_numpy(self.np_params[g]).to(dev).requires_grad_(True)))
        groups = [{"params": [getattr(self, a)], "lr": 1e-3, "name": n} for n, a in ATTR.items()]
        self.optimizer = (FusedAdam if optimizer == "fused" else torch.optim.Adam)(groups, lr=0.0, eps=1e-15)
        if with_state:
            self.take_step(seed)
        self.xyz_gradient_accum = torch.ones((P, 1), device=dev)
        self.denom = torch.ones((P, 1), device=dev)
        self.max_radii2D = torch.ones((P,), device=dev)

    def take_step(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        for a in ATTR.values():
            p = getattr(self, a)
            p.grad = torch.randn(p.shape, generator=g).to(p.device)
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)

    def snapshot(self):
        """{name: numpy} of the six parameters and, where they exist, both moments."""
        out = {g: getattr(self, a).detach().cpu().numpy().copy() for g, a in ATTR.items()}
        for g, a in ATTR.items():
            st = self.optimizer.state.get(getattr(self, a), {})
            for key in ("exp_avg", "exp_avg_sq"):
                if key in st:
                    out[f"{g}.{key}"] = st[key].detach().cpu().numpy().copy()
        return out


def split_snapshot(snap):
    return {g: snap[g] for g in GROUPS}, {k: v for k, v in snap.items() if "." in k}


@pytest.mark.parametrize("optimizer", ["fused", "torch"])
@pytest.mark.parametrize("cap_max, n_new", [(1020, 20), (5000, 50), (1000, 0)])
def test_grow(hip_device, optimizer, cap_max, n_new):
    """Tolerance as in test_relocate_against_the_reference, measured for this test's rows.  Recorded (float32 restatement / bar /
    device): cap 1020 opacity 3.74e-06 / 1.49e-05 / 3.74e-06, scaling 3.00e-07 / 1.20e-06 / 9.15e-07; cap 5000 opacity
    6.78e-06 / 2.71e-05 / 7.01e-06, scaling 3.27e-07 / 1.31e-06 / 1.08e-06 (the device's expf and logf are a few ulp of the
    log-scale, ~4e-7 each at -5, off the host's)."""
    from luciddreamer_amd import mcmc
    P = 1000
    model = Model(P, hip_device, seed=7, optimizer=optimizer)
    before = model.snapshot()
    objects = [getattr(model, a) for a in ATTR.values()]
    s = mcmc.MCMCStrategy(cap_max, min_opacity=MIN_OPACITY)
    assert s.n_new(P) == n_new
    src = np.random.default_rng(cap_max).integers(0, P, n_new)
    src[: n_new // 2] = src[0] if n_new else 0                         # one source many times
    added = s.grow(model, sampled_idx=torch.from_numpy(src).to(hip_device))
    assert added == n_new and model._xyz.shape[0] == P + n_new
    after = model.snapshot()
    if n_new == 0:
        assert all(a is b for a, b in zip(objects, (getattr(model, a) for a in ATTR.values())))
        assert before.keys() == after.keys()
        for k in before:
            assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
        return
    st = model._lr_store
    assert st.P == P + n_new
    for g, a in ATTR.items():
        p = getattr(model, a)
        assert p.shape[0] == P + n_new and p.data_ptr() == st.bufs[g].data_ptr() and p.requires_grad
        assert {gr["name"]: gr for gr in model.optimizer.param_groups}[g]["params"][0] is p
        for key in ("exp_avg", "exp_avg_sq"):
            m = model.optimizer.state[p][key]
            assert m.shape == p.shape and m.data_ptr() == st.bufs[f"{g}.{key}"].data_ptr(), (g, key)
    for a in ("xyz_gradient_accum", "denom", "max_radii2D"):
        t = getattr(model, a)
        assert t.shape[0] == P + n_new and not t[P:].any() and bool((t[:P] == 1).all()), a
    # the reference on the same rows: the old tensors with n_new empty rows behind them
    pad = lambda v: np.concatenate((v, np.zeros((n_new,) + v.shape[1:], np.float32)))
    params, moments = split_snapshot({k: pad(v) for k, v in before.items()})
    dst = np.arange(P, P + n_new)
    ref64, mom_ref = R.relocate(params, moments, dst, src, MIN_OPACITY, 51)
    ref32, _ = R.relocate(params, None, dst, src, MIN_OPACITY, 51, dtype=np.float32)
    touched = np.unique(np.concatenate((dst, src)))
    bar = bars(ref64, ref32, touched)
    for k in ("xyz", "f_dc", "f_rest", "rotation"):
        assert np.array_equal(after[k].view(np.uint32), ref64[k].view(np.uint32)), k          # new rows are copies, old rows intact
    for k in ("opacity", "scaling"):
        untouched = np.setdiff1d(np.arange(P), touched)
        assert np.array_equal(after[k][untouched].view(np.uint32), before[k][untouched].view(np.uint32)), k
        assert not np.array_equal(after[k][np.unique(src)], before[k][np.unique(src)]), k       # sources are updated
        err = float(np.abs(after[k][touched].astype(np.float64) - ref64[k][touched]).max())
        print(f"grow cap={cap_max} {k}: float32 restatement {bar[k][0]:.3e}  bar {bar[k][1]:.3e}  device {err:.3e}")
        assert err <= bar[k][1], (k, err, bar[k])
    for k in mom_ref:
        assert np.array_equal(after[k], mom_ref[k]), k                                         # zero at touched rows, else intact
    # the optimizer keeps working on the re-pointed tensors
    xyz_before = model._xyz.detach().clone()
    model.take_step(seed=3)
    assert model._xyz.shape[0] == P + n_new and not torch.equal(model._xyz.detach(), xyz_before)
    assert all(torch.isfinite(getattr(model, a)).all() for a in ATTR.values())


def test_relocate_through_the_strategy(hip_device):
    from luciddreamer_amd import mcmc
    P = 1000
    model = Model(P, hip_device, seed=21)
    before = model.snapshot()
    o = R.sigmoid(before["opacity"].astype(np.float64)).reshape(-1)
    dead, alive = np.nonzero(o <= MIN_OPACITY)[0], np.nonzero(o > MIN_OPACITY)[0]
    assert len(dead) > 20
    s = mcmc.MCMCStrategy(P, min_opacity=MIN_OPACITY)
    gen = torch.Generator(device=hip_device).manual_seed(5)
    assert s.relocate(model, generator=gen) == len(dead)
    after = model.snapshot()
    assert model._xyz.shape[0] == P
    assert not bool((torch.sigmoid(model._opacity.detach()) < MIN_OPACITY).any())
    alive_xyz = {before["xyz"][i].tobytes() for i in alive}
    assert all(after["xyz"][i].tobytes() in alive_xyz for i in dead)
    assert np.array_equal(after["xyz"][alive], before["xyz"][alive])
    assert s.relocate(model, generator=gen) == 0                                  # nothing is dead any more
    # explicit sources: the strategy is the direct call on the same rows
    model2 = Model(P, hip_device, seed=21)
    src = alive[np.random.default_rng(1).integers(0, len(alive), len(dead))]
    assert s.relocate(model2, sampled_idx=torch.from_numpy(src).to(hip_device)) == len(dead)
    params, moments = split_snapshot(before)
    want, want_m = run_relocate(params, moments, dead, src, hip_device)
    got = model2.snapshot()
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    for k in want_m:
        assert np.array_equal(got[k].view(np.uint32), want_m[k].view(np.uint32)), k
    with pytest.raises(RuntimeError, match="dead row"):
        s.relocate(Model(P, hip_device, seed=21), sampled_idx=torch.from_numpy(np.full(len(dead), dead[0])).to(hip_device))


# ---- position noise -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 64, 65, 1037])
def test_noise_against_the_reference(hip_device, P):
    """Distance = max |xyz' - reference| / max |delta| of the case.  Recorded on an MI355X with this file (float32 restatement
    on the CPU / bar = 4 x / device): P = 1 9.28e-07 / 3.71e-06 / 1.19e-06, P = 64 1.03e-06 / 4.11e-06 / 8.24e-07,
    P = 65 6.37e-07 / 2.55e-06 / 6.75e-07, P = 1037 1.23e-06 / 4.92e-06 / 1.23e-06."""
    from luciddreamer_amd import mcmc
    params = make_params(P, seed=100 + P)
    params["opacity"][0, 0] = np.float32(logit(0.004))                 # row 0 always moves (the gate is ~0.5 there)
    noise = torch.randn((P, 3), generator=torch.Generator().manual_seed(P)).numpy()
    scaler = 5e5 * 1.6e-4
    args = (params["scaling"], params["rotation"], params["opacity"], noise, scaler)
    ref64 = R.noise_step(params["xyz"], *args)
    ref32 = R.noise_step(params["xyz"], *args, dtype=np.float32)
    scale = float(np.abs(R.noise_delta(*args)).max())
    assert scale > 0
    e32 = float(np.abs(ref32.astype(np.float64) - ref64).max()) / scale
    d = to_dev(params, hip_device)
    xyz = d["xyz"].clone()
    mcmc.add_noise(xyz, d["scaling"], d["rotation"], d["opacity"], torch.from_numpy(noise).to(hip_device), scaler)
    got = xyz.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - ref64).max()) / scale
    print(f"noise P={P}: float32 restatement {e32:.3e}  bar {4 * e32:.3e}  device {err:.3e}  (max |delta| {scale:.3e})")
    assert err <= 4 * e32, (err, e32)
    opaque = R.sigmoid(params["opacity"].astype(np.float64)).reshape(-1) >= 0.5
    moved = np.abs(got[opaque].astype(np.float64) - params["xyz"][opaque])
    assert moved.size == 0 or float(moved.max()) < 1e-30                # exactly 0.0f, or a denormal's worth
    # no noise, no movement: the bits stay
    xyz0 = d["xyz"].clone()
    mcmc.add_noise(xyz0, d["scaling"], d["rotation"], d["opacity"], torch.zeros((P, 3), device=hip_device), scaler)
    assert np.array_equal(xyz0.cpu().numpy().view(np.uint32), params["xyz"].view(np.uint32))


def test_inject_noise_through_the_strategy(hip_device):
    from luciddreamer_amd import mcmc
    model = Model(257, hip_device, seed=4, with_state=False)
    s = mcmc.MCMCStrategy(1000, noise_lr=5e5)
    noise = torch.randn((257, 3), generator=torch.Generator().manual_seed(0)).to(hip_device)
    want = model._xyz.detach().clone()
    mcmc.add_noise(want, model._scaling.detach(), model._rotation.detach(), model._opacity.detach(), noise, 5e5 * 1.6e-4)
    s.inject_noise(model, 1.6e-4, noise=noise)
    assert torch.equal(model._xyz.detach(), want) and not torch.equal(want, torch.from_numpy(model.np_params["xyz"]).to(hip_device))
    gen = torch.Generator(device=hip_device).manual_seed(2)
    s.inject_noise(model, 1.6e-4, generator=gen)
    assert torch.isfinite(model._xyz).all() and not torch.equal(model._xyz.detach(), want)


# ---- regularisers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 257])
def test_regulariser_gradients_are_added(hip_device, P):
    """Against autograd of opacity_reg mean(sigmoid(o)) + scale_reg mean(exp(s)) in float64 on the host, with gradients of the
    regularisers' own magnitude already in the buffers; distance = max |g' - reference|, bar = 4 x the float32 restatement's.
    Recorded (restatement / bar / device): P = 1 opacity 3.39e-11 / 1.36e-10 / 3.39e-11, scaling 2.69e-11 / 1.08e-10 / 5.90e-11;
    P = 257 opacity 4.00e-12 / 1.60e-11 / 4.00e-12, scaling 6.26e-13 / 2.51e-12 / 3.68e-13."""
    from luciddreamer_amd import mcmc
    params = make_params(P, seed=300 + P)
    w_o, w_s = 0.01, 0.01
    o64 = torch.from_numpy(params["opacity"]).double().requires_grad_(True)
    s64 = torch.from_numpy(params["scaling"]).double().requires_grad_(True)
    (w_o * torch.sigmoid(o64).mean() + w_s * torch.exp(s64).mean()).backward()
    rng = np.random.default_rng(P)
    g_o = (rng.normal(size=(P, 1)) * 1e-2 / P).astype(np.float32)
    g_s = (rng.normal(size=(P, 3)) * 1e-4 / P).astype(np.float32)
    want = {"opacity": g_o.astype(np.float64) + o64.grad.numpy(), "scaling": g_s.astype(np.float64) + s64.grad.numpy()}
    r_o, r_s = R.reg_grad(params["opacity"], params["scaling"], w_o, w_s)
    assert np.allclose(r_o, o64.grad.numpy(), rtol=1e-12, atol=0) and np.allclose(r_s, s64.grad.numpy(), rtol=1e-12, atol=0)
    f_o, f_s = R.reg_grad(params["opacity"], params["scaling"], w_o, w_s, dtype=np.float32)
    f32 = {"opacity": g_o + f_o, "scaling": g_s + f_s}
    d = to_dev(params, hip_device)
    got_o, got_s = torch.from_numpy(g_o).to(hip_device), torch.from_numpy(g_s).to(hip_device)
    mcmc.add_reg_grad(d["opacity"], d["scaling"], w_o, w_s, got_o, got_s)
    got = {"opacity": got_o.cpu().numpy(), "scaling": got_s.cpu().numpy()}
    for k in want:
        e32 = float(np.abs(f32[k].astype(np.float64) - want[k]).max())
        err = float(np.abs(got[k].astype(np.float64) - want[k]).max())
        print(f"reg_grad P={P} {k}: float32 restatement {e32:.3e}  bar {4 * e32:.3e}  device {err:.3e}")
        assert err <= 4 * e32, (k, err, e32)
        assert float(np.abs(got[k] - (g_o if k == "opacity" else g_s)).max()) > 0      # something was added ...
    # ... through the strategy too, into .grad (created when absent)
    model = Model(P, hip_device, seed=300 + P, with_state=False)
    model._opacity.grad = torch.from_numpy(g_o).to(hip_device)
    mcmc.MCMCStrategy(1000, opacity_reg=w_o, scale_reg=w_s).add_regularizer_grads(model)
    assert torch.equal(model._opacity.grad, got_o)
    assert model._scaling.grad is not None and bool((model._scaling.grad > 0).all())


# ---- one short loop -------------------------------------------------------------------------------------------------------
def test_short_training_loop_under_the_cap(hip_device):
    """2000 Gaussians, 64x64, 4 views, 120 iterations of render_raw + l1_dssim_loss + FusedAdam + MCMCStrategy: the count
    climbs 5 % per refinement to the cap and stays there, nothing is dead right after a refinement, everything stays finite and
    no render reports an overflow.  No assertion on the loss value."""
    import importlib.util
    from luciddreamer_amd import config, mcmc
    from luciddreamer_amd.gaussian_renderer import render_raw
    from luciddreamer_amd.loss import l1_dssim_loss
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "train_loop.py")
    spec = importlib.util.spec_from_file_location("train_loop_example_mcmc", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.default_args(gaussians=4000, resolution="64x64", views=4)            # the loop starts from every second Gaussian
    model, cams, targets = mod.build(args, hip_device)
    assert model._xyz.shape[0] == 2000
    bg = torch.zeros(3, device=hip_device)
    s = mcmc.MCMCStrategy(cap_max=2300, refine_start=20, refine_every=20)
    gen = torch.Generator(device=hip_device).manual_seed(0)
    config.set_async(True, headroom=1.5, warm_calls=len(cams))
    reports = (config.rerendered_views, config.dropped_views)
    counts = []
    try:
        for it in range(1, 121):
            pkg = render_raw(cams[it % len(cams)], model, bg_color=bg)
            l1_dssim_loss(pkg["render"], targets[it % len(cams)], 0.2).backward()
            s.add_regularizer_grads(model)
            model.optimizer.step()
            model.optimizer.zero_grad(set_to_none=True)
            moved, added = s.step(model, it, 1.6e-4, generator=gen)
            P = int(model._xyz.shape[0])
            counts.append(P)
            assert P <= 2300
            if it >= 20 and it % 20 == 0:
                assert not bool((torch.sigmoid(model._opacity.detach()) <= s.min_opacity).any()), it
            else:
                assert moved == 0 and added == 0
        config.drain()
        assert (config.rerendered_views, config.dropped_views) == reports
    finally:
        config.set_async(True)
        config.reset()
    assert counts[18] == 2000 and counts[19] == 2100 and counts[-1] == 2300 and sorted(counts) == counts
    for a in ATTR.values():
        assert torch.isfinite(getattr(model, a)).all(), a
