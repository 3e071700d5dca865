"""The references of tests/adam_ref.py checked on the CPU: adam_step_ref against torch.optim.Adam in float64, the mirror of
common.h's geom_layout against lr_geom_bytes, select_ref and pack_ply_ref on hand-written cases."""
import pytest
import torch

from tests import adam_ref as R


def _worst_rel(steps_with_lr, zero_rows):
    g = torch.Generator().manual_seed(11)
    shapes = [(257, 3), (64, 15, 3), (1,), (33, 4)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-3} for p in ps], lr=0.0, eps=1e-15)
    ref = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    worst = 0.0
    for step, lr in enumerate(steps_with_lr, start=1):
        for grp in opt.param_groups:
            grp["lr"] = lr
        for k, p in enumerate(ps):
            gr = torch.randn(p.shape, generator=g, dtype=torch.float64) * 10.0 ** (k - 2)
            if zero_rows and p.dim() > 1:
                gr[step % 3::3] = 0                                     # rows that were not visible this step
            p.grad = gr
            ref[k] = R.adam_step_ref(*ref[k][:1], gr, *ref[k][1:], lr, 0.9, 0.999, 1e-15, step)
        opt.step()
        for k, p in enumerate(ps):
            st = opt.state[p]
            for got, want in zip(ref[k], (p.detach(), st["exp_avg"], st["exp_avg_sq"])):
                assert got.dtype == torch.float64
                worst = max(worst, float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()))
    return worst


def test_reference_is_torch_adam_in_float64():
    """Five steps, the learning rate changed after the second, rows with zero gradient on every step: the reference and
    torch.optim.Adam differ by float64 rounding only (torch fuses lerp / addcmul / addcdiv, the reference does not)."""
    worst = _worst_rel([1e-3, 1e-3, 2.5e-4, 2.5e-4, 2.5e-4], zero_rows=True)
    # measured: 7.7e-14, the largest ELEMENTWISE relative difference over parameters and both moments of all five steps (a few
    # hundred float64 ulps: it is taken at a parameter that an update has brought close to zero, where the rounding of the
    # update is divided by what the cancellation left); the bound is one decade above
    assert worst <= 7.7e-13, worst


def test_reference_stays_finite_where_nothing_was_ever_visited():
    """Gradient and both moments zero (an all-zero visibility mask from the first step on): 0 / (0 + eps) is 0, the parameters
    keep their values, signed zeros included."""
    p = torch.tensor([1.5, -0.0, 0.0, -3.0e-30], dtype=torch.float32)
    m = v = torch.zeros(4)
    for step in (1, 2, 3):
        p2, m2, v2 = R.adam_step_ref(p, torch.zeros(4), m, v, 0.05, 0.9, 0.999, 1e-15, step)
        assert all(bool(torch.isfinite(t).all()) for t in (p2, m2, v2))
        assert torch.equal(p2, p.double()) and not bool(m2.any()) and not bool(v2.any())
        assert torch.equal(torch.signbit(p2), torch.signbit(p))


@pytest.fixture(scope="module")
def built_lib():
    from luciddreamer_amd import build
    return build.build()


@pytest.mark.parametrize("P", [1, 3, 1021, 4099, 93_337])
def test_mirror_of_the_geom_layout_gives_the_library_size(built_lib, P):
    from luciddreamer_amd import _lib
    a = R.align256
    assert 256 + a(48 * P) + a(P) + 3 * a(4 * P) + a(16 * P) == _lib.lib().lr_geom_bytes(P) == R.geom_bytes(P)
    assert R.tiles_touched_offset(P) == 256 + a(48 * P) + a(P)


def test_select_reference_on_hand_written_cases():
    src = torch.tensor([[10, 11], [20, 21], [30, 31], [40, 41]], dtype=torch.int32)
    sent = torch.full((7, 2), -1, dtype=torch.int32)
    dst, n = R.select_ref(src, torch.tensor([0, 2, 0, 255], dtype=torch.uint8), sent, 0)      # any non-zero byte selects
    assert n == 2 and dst.tolist() == [[20, 21], [40, 41], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]
    dst, n = R.select_ref(src, torch.tensor([1, 1, 0, 1], dtype=torch.uint8), sent, 3)        # appended behind three rows
    assert n == 3 and dst.tolist() == [[-1, -1], [-1, -1], [-1, -1], [10, 11], [20, 21], [40, 41], [-1, -1]]
    dst, n = R.select_ref(src, torch.zeros(4, dtype=torch.uint8), sent, 5)
    assert n == 0 and torch.equal(dst, sent) and torch.equal(sent, torch.full((7, 2), -1, dtype=torch.int32))


def test_pack_ply_reference_on_a_hand_written_case():
    """One vertex, two rest coefficients: f_rest [1,2,3] = [[r0 g0 b0], [r1 g1 b1]] goes out channel-major r0 r1 g0 g1 b0 b1."""
    row = R.pack_ply_ref(torch.tensor([[1., 2., 3.]]), torch.tensor([[[4., 5., 6.]]]),
                         torch.tensor([[[10., 20., 30.], [11., 21., 31.]]]), torch.tensor([[7.]]),
                         torch.tensor([[8., 9., 10.]]), torch.tensor([[.1, .2, .3, .4]]))
    assert row.tolist() == [[1., 2., 3., 0., 0., 0., 4., 5., 6., 10., 11., 20., 21., 30., 31., 7., 8., 9., 10.,
                             pytest.approx(.1), pytest.approx(.2), pytest.approx(.3), pytest.approx(.4)]]
    none = R.pack_ply_ref(torch.ones(2, 3), torch.ones(2, 1, 3), torch.ones(2, 0, 3), torch.ones(2, 1), torch.ones(2, 3),
                          torch.ones(2, 4))
    assert none.shape == (2, 17)
