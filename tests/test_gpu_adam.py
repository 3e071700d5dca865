"""csrc/adam.hip on the branches that sizes and shapes choose: the masked step (lr_adam_step_masked through _C.adam_step_masked)
on its scalar tail, its run-time row length, mixed float4 groups, the overflow branch and the grid-stride continuation, against
the unmasked step (the SAME BITS, include/lucid_raster.h) and against the float64 reference of tests/adam_ref.py; the unmasked
step's grid-stride continuation and FusedAdam.step's chunking against torch.optim.Adam."""
import ctypes

import pytest
import torch
import torch.nn as nn

from tests import adam_ref as R

pytestmark = pytest.mark.gpu
B1, B2, EPS = 0.9, 0.999, 1e-15
# per Gaussian: the four compile-time row lengths (1, 3, 4, 45), the run-time path (9, 24, 7, 2) and one empty tensor (the
# binding drops it: features_rest of a degree-0 model); sixteen slots = one full launch
ROWS = [(1,), (3,), (4,), (1, 3), (15, 3), (3, 3), (8, 3), (7,), (2,), (0, 3), (3,), (1,), (15, 3), (4,), (8, 3), (3, 3)]
LRS = [1e-2, 1.6e-3, 1e-3, 2.5e-3, 1.25e-3, 5e-3, 2e-3, 9e-3, 3e-3, 1e-3, 4e-3, 3.5e-3, 1.5e-3, 6e-3, 7e-3, 8e-3]
PATTERNS = ("none", "all", "first", "last", "alternating", "third", "bernoulli05", "bernoulli5")


def _pattern(name, P, seed):
    i = torch.arange(P)
    if name == "none":
        return torch.zeros(P, dtype=torch.bool)
    if name == "all":
        return torch.ones(P, dtype=torch.bool)
    if name == "first":
        return i == 0
    if name == "last":
        return i == P - 1
    if name == "alternating":
        return i % 2 == 1
    if name == "third":
        return i % 3 == 0
    prob = {"bernoulli05": 0.05, "bernoulli5": 0.5, "bernoulli3": 0.3}[name]
    return torch.rand(P, generator=torch.Generator().manual_seed(seed)) < prob


def _touched(mask):
    """tiles_touched of a view that visits the Gaussians of `mask`: any non-zero count means visited."""
    P = mask.numel()
    return torch.tensor([1, 7, 40_000])[torch.arange(P) % 3] * mask.to(torch.int64)


def _adam_unmasked(ps, gs, ms, vs, lrs, step):
    from luciddreamer_amd import _lib
    n = len(ps)
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    numel = (ctypes.c_ulonglong * n)(*[t.numel() for t in ps])
    dev = ps[0].device
    with _lib.on_device(dev):
        rc = _lib.lib().lr_adam_step(n, arr(ps), arr(gs), arr(ms), arr(vs), numel, (ctypes.c_double * n)(*lrs), B1, B2, EPS,
                                     int(step), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc


def _bits(t):
    return t.contiguous().view(torch.int32)


def _close(got, want):
    """The bound of test_gpu_optim.test_matches_torch_adam: max abs difference <= 2e-6 * max |reference| per tensor."""
    got = got.detach().cpu().double()
    return bool(torch.isfinite(got).all()) and float((got - want).abs().max()) <= 2e-6 * float(want.abs().max())


def _masked_against_unmasked_and_reference(dev, P, masks, overflow=None, shapes=ROWS, lrs=LRS, seed=0):
    """One step per entry of `masks` from zero moments.  A takes lr_adam_step_masked with NaN in every gradient row the step
    must not read, B takes lr_adam_step with zeros there, the reference takes B's gradients in float64."""
    from luciddreamer_amd import _C
    overflow = overflow or [0] * len(masks)
    gen = torch.Generator().manual_seed(1000 * seed + P)
    effective = [m & (o == 0) for m, o in zip(masks, overflow)]            # an overflowed view visits nothing
    never = ~torch.stack(effective).any(0)
    p0 = [torch.randn((P,) + s, generator=gen) for s in shapes]
    for t in p0:
        if t.numel():
            rows = t.view(P, -1)
            rows[never, ::2] = -0.0                                          # signed zeros where nothing will ever arrive
            rows[2::5, ::2] = -0.0                                           # ... and among rows that move
    A = [[t.to(dev) for t in p0], [torch.zeros_like(t, device=dev) for t in p0], [torch.zeros_like(t, device=dev) for t in p0]]
    B = [[t.clone() for t in part] for part in A]
    ref = [(t.double(), torch.zeros_like(t, dtype=torch.float64), torch.zeros_like(t, dtype=torch.float64)) for t in p0]
    live = [k for k, t in enumerate(p0) if t.numel()]
    prev = None
    for step, (mask, eff, ovf) in enumerate(zip(masks, effective, overflow), start=1):
        grads = [torch.randn(t.shape, generator=gen) for t in p0]
        row = lambda t: eff.view((P,) + (1,) * (t.dim() - 1))
        g_zero = [torch.where(row(g), g, torch.zeros(())) for g in grads]
        g_nan = [torch.where(row(g), g, torch.full((), float("nan"))) for g in grads]
        geom = R.masked_geom(P, _touched(mask), ovf, dev)
        _C.adam_step_masked(A[0], [g.to(dev) for g in g_nan], A[1], A[2], list(lrs), B1, B2, EPS, step, geom)
        _adam_unmasked(B[0], [g.to(dev) for g in g_zero], B[1], B[2], lrs, step)
        ref = [R.adam_step_ref(ref[k][0], g_zero[k], ref[k][1], ref[k][2], lrs[k], B1, B2, EPS, step) for k in range(len(p0))]
        wrong = []                                   # every (slot, row shape, array) that misses, not only the first
        for k in live:
            for part, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
                if not torch.equal(_bits(A[part][k]), _bits(B[part][k])):                      # (a) the bits of the unmasked step
                    wrong.append(f"slot {k} {shapes[k]} {name}: bits differ from lr_adam_step")
                if not (_close(A[part][k], ref[k][part]) and _close(B[part][k], ref[k][part])):    # (b)
                    wrong.append(f"slot {k} {shapes[k]} {name}: off the float64 reference")
        assert not wrong, f"P = {P}, step {step}: " + "; ".join(wrong)
        if step == 2:
            # visited at step 1 and not at step 2: the moments decay and the parameter keeps moving
            gone = effective[0] & ~effective[1]
            for k in live:
                for part in range(3):
                    now, before = A[part][k].cpu().view(P, -1)[gone], prev[part][k].view(P, -1)[gone]
                    assert bool((now != before).all()), (P, shapes[k], part)
                m_now, m_before = A[1][k].cpu().view(P, -1)[gone], prev[1][k].view(P, -1)[gone]
                assert bool((m_now.abs() < m_before.abs()).all())
        prev = [[t.cpu().clone() for t in part] for part in A]
    for k in live:                                   # never visited, zero moments: not one bit changes (-0.0 stays -0.0)
        assert torch.equal(_bits(A[0][k].cpu().view(P, -1)[never]), _bits(p0[k].view(P, -1)[never])), shapes[k]
        for part in (1, 2):
            assert not bool(_bits(A[part][k].cpu().view(P, -1)[never]).any()), shapes[k]
    return never, effective


@pytest.mark.parametrize("first", range(len(PATTERNS)))
@pytest.mark.parametrize("P", [1, 2, 3, 5, 1021, 4099])
def test_masked_step_is_the_unmasked_step_on_every_row_length_and_tail(hip_device, P, first):
    """No P is a multiple of 4: the scalar tail of every tensor with an odd row length runs, and P < 4 leaves some tensors
    without one float4 group.  Row lengths 3, 9, 24, 45 and 7 put Gaussians of opposite visibility into one float4 group under
    the alternating and every-third masks.  Three steps with three different masks; each of the eight patterns is the first,
    the second and the third step of some case."""
    names = [PATTERNS[(first + d) % len(PATTERNS)] for d in (0, 1, 3)]
    masks = [_pattern(n, P, seed=17 * first + s) for s, n in enumerate(names)]
    never, effective = _masked_against_unmasked_and_reference(hip_device, P, masks, seed=first)
    if P == 4099 and names[0] == "all":
        assert int((effective[0] & ~effective[1]).sum()) == P - 1          # the decay check above had rows to look at
    if P == 4099 and names == ["first", "last", "alternating"]:
        assert int(never.sum()) == 2049                                      # ... and so had the never-visited check


@pytest.mark.parametrize("P", [5, 4099])
def test_overflowed_view_takes_every_gradient_as_zero_without_reading_it(hip_device, P):
    """GeomHeader::overflow = 1 with tiles_touched all non-zero and a gradient array that is NaN throughout: a step of zero
    gradients.  First on zero moments (nothing moves), then after a real step (everything decays)."""
    everyone = torch.ones(P, dtype=torch.bool)
    never, _ = _masked_against_unmasked_and_reference(hip_device, P, [everyone, everyone, everyone], overflow=[1, 0, 1], seed=9)
    assert not bool(never.any())


def test_masked_step_beyond_one_grid_of_4096_workgroups(hip_device):
    """93,337 x 45 = 4,200,165 elements: more than the 4 * 4096 * 256 the capped grid covers in one turn, and 1 mod 4."""
    P = 93_337
    assert P * 45 > 4 * 4096 * 256 and (P * 45) % 4 == 1
    _masked_against_unmasked_and_reference(hip_device, P, [_pattern("bernoulli3", P, seed=5)], shapes=[(15, 3), (3,)],
                                           lrs=[1.25e-3, 1.6e-3], seed=3)


def _against_torch_adam(hip_device, sizes, steps, skip=None, seed=0):
    """FusedAdam and torch.optim.Adam over the same parameters and gradients; skip(step, k): parameter k has no gradient."""
    from luciddreamer_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=g) for n in sizes]
    a = [nn.Parameter(t.to(hip_device)) for t in init]
    b = [nn.Parameter(t.to(hip_device)) for t in init]
    ref = torch.optim.Adam(a, lr=1e-2, eps=1e-15)
    fus = FusedAdam(b, lr=1e-2, eps=1e-15)
    taken = [0] * len(sizes)
    for step in range(steps):
        for k, (x, y) in enumerate(zip(a, b)):
            gr = torch.randn(x.shape, generator=g).to(hip_device)
            if skip is not None and skip(step, k):
                x.grad = y.grad = None
            else:
                x.grad, y.grad = gr.clone(), gr.clone()
                taken[k] += 1
        ref.step()
        fus.step()
    close = lambda got, want: float((got - want).abs().max()) <= 2e-6 * float(want.abs().max())
    for k, (x, y) in enumerate(zip(a, b)):
        assert int(ref.state[x]["step"]) == int(fus.state[y]["step"]) == taken[k], k
        if x.numel() == 0:
            continue
        assert not torch.equal(y.detach().cpu(), init[k]), k
        assert close(y.detach(), x.detach()), (k, sizes[k])
        assert close(fus.state[y]["exp_avg"], ref.state[x]["exp_avg"]), (k, sizes[k])
        assert close(fus.state[y]["exp_avg_sq"], ref.state[x]["exp_avg_sq"]), (k, sizes[k])


def test_unmasked_step_beyond_one_grid_of_4096_workgroups(hip_device):
    _against_torch_adam(hip_device, [4_200_165], steps=3)


CHUNK_SIZES = [1, 3, 1021, 4103, 0, 4103, 1, 1021, 3, 3, 1021, 1, 4103, 3, 1, 1021, 4103, 3, 1021, 1]


def test_twenty_parameters_take_two_launches(hip_device):
    """16 + 4 tensors, one of them (and its gradient) without elements."""
    assert len(CHUNK_SIZES) == 20 and CHUNK_SIZES.count(0) == 1
    _against_torch_adam(hip_device, CHUNK_SIZES, steps=3, seed=1)


def test_parameters_that_skip_a_step_are_batched_by_their_own_step_count(hip_device):
    """Every second parameter has no gradient on the second step: from then on the step counts differ and one step() makes one
    launch per count, each with its own bias corrections."""
    _against_torch_adam(hip_device, CHUNK_SIZES, steps=3, skip=lambda step, k: step == 1 and k % 2 == 0, seed=2)


def test_tiles_touched_sits_where_the_mirror_says(hip_device):
    """One real forward: what masked_geom writes at tiles_touched_offset(P) is what the library keeps there -- the instances
    each Gaussian emits.  Its non-zero entries are the emitting Gaussians (header word 8), its sum the instances (word 6),
    and nothing emits without a radius."""
    from tests import helpers as hp
    from tests.test_gpu_full import _raw_forward
    P, W, H = 3000, 160, 96
    cam, cloud = hp.box_setup(P, W, H)
    out = _raw_forward(cloud, cam, 3, torch.zeros(3), hip_device)
    radii, geom = out[3].cpu(), out[4].cpu()
    assert geom.numel() == R.geom_bytes(P)
    hdr = geom[:256].view(torch.int32)
    off = R.tiles_touched_offset(P)
    touched = geom[off:off + 4 * P].view(torch.int32).to(torch.int64)
    assert int(hdr[4]) == P and int(hdr[1]) == 0
    assert int((touched != 0).sum()) == int(hdr[8]) > 0
    assert int(touched.sum()) == int(hdr[6]) > 0
    assert bool((radii[touched != 0] > 0).all())
