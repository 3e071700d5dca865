"""csrc/rows.hip called through the C ABI: lr_select_rows (k_mask_count, k_mask_rank, k_gather_rows) at the sizes where its
loops take another turn and at masks that sit on its 128-row and 2048-row borders, and lr_pack_ply_rows at every SH degree.
Byte movement: the data are random int32 bit patterns (NaN encodings among them) and every comparison is of integers."""
import ctypes

import pytest
import torch

from tests import adam_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -1_234_567_891
GUARD = 64                      # sentinel rows in front of the destination pointer and behind the last row a call may write
MASKS = ("zeros", "ones", "first", "last", "2047_2048", "block_ends", "one_tile", "alternating", "bernoulli01", "bernoulli99",
         "values_0_2_255")


def _mask(name, P, gen):
    i = torch.arange(P)
    if name == "zeros":
        m = torch.zeros(P, dtype=torch.bool)
    elif name == "ones":
        m = torch.ones(P, dtype=torch.bool)
    elif name == "first":
        m = i == 0
    elif name == "last":
        m = i == P - 1
    elif name == "2047_2048":
        m = (i == 2047) | (i == 2048)                   # the last row of one k_mask_rank workgroup and the first of the next
    elif name == "block_ends":
        m = i % 128 == 127                              # the last row of every k_gather_rows workgroup
    elif name == "one_tile":
        m = i < 2048                                    # one full workgroup of ones, then nothing
    elif name == "alternating":
        m = i % 2 == 0
    elif name == "bernoulli01":
        m = torch.rand(P, generator=gen) < 0.01
    elif name == "bernoulli99":
        m = torch.rand(P, generator=gen) < 0.99
    elif name == "values_0_2_255":
        return torch.tensor([0, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, (P,), generator=gen)]
    else:
        raise ValueError(name)
    return m.to(torch.uint8)


def _select(dev, P, mask, src_ptrs, dst_ptrs, row_bytes, off, ws):
    """One lr_select_rows call with out_count preset to -7; returns the count it wrote."""
    from luciddreamer_amd import _lib
    L = _lib.lib()
    n = len(src_ptrs)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    assert ws.numel() >= L.lr_select_workspace_bytes(P)
    with _lib.on_device(dev):
        rc = L.lr_select_rows(P, mask.data_ptr(), n, (ctypes.c_void_p * n)(*src_ptrs), (ctypes.c_void_p * n)(*dst_ptrs),
                              (ctypes.c_uint * n)(*row_bytes), off, cnt.data_ptr(), ws.data_ptr(), ws.numel(),
                              torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    return int(cnt.item())


def _dirty_workspace(dev, P):
    from luciddreamer_amd import _lib
    return torch.full((_lib.lib().lr_select_workspace_bytes(P),), 0xFF, dtype=torch.uint8, device=dev)


_sources = {}


def _source(dev, P, row_bytes):
    """Random bit patterns [P, row_bytes / 4] per tensor, made once per (P, widths) and never written."""
    key = (P, tuple(row_bytes))
    if key not in _sources:
        gen = torch.Generator().manual_seed(P)
        _sources[key] = [torch.randint(-2 ** 31, 2 ** 31, (P, rb // 4), generator=gen, dtype=torch.int64).to(torch.int32).to(dev)
                         for rb in row_bytes]
        nan_bits = torch.tensor([0x7FC00000, -0x00400000, 0x7F800001], dtype=torch.int32, device=dev)     # quiet, negative, signalling
        for t in _sources[key]:
            t.view(-1)[::97] = nan_bits[torch.arange(t.view(-1)[::97].numel(), device=dev) % 3]
    return _sources[key]


def _check_select(dev, P, row_bytes, mask_names, offsets, seed=0):
    gen = torch.Generator().manual_seed(seed * 7919 + P)
    src = _source(dev, P, row_bytes)
    ws = _dirty_workspace(dev, P)
    for name in mask_names:
        mask_cpu = _mask(name, P, gen)
        mask = mask_cpu.to(dev)
        want_n = int((mask_cpu != 0).sum())
        for off in offsets:
            ws.fill_(0xFF)
            rows = GUARD + off + want_n + GUARD
            sent = [torch.full((rows, rb // 4), SENTINEL, dtype=torch.int32, device=dev) for rb in row_bytes]
            dst = [s.clone() for s in sent]
            got_n = _select(dev, P, mask, [t.data_ptr() for t in src], [d[GUARD:].data_ptr() for d in dst], row_bytes, off, ws)
            assert got_n == want_n, (P, name, off, got_n, want_n)
            for t, d, s, rb in zip(src, dst, sent, row_bytes):
                want, _ = R.select_ref(t, mask, s, GUARD + off)
                assert torch.equal(d, want), (P, name, off, rb)


SMALL_P = [1, 127, 128, 129, 2047, 2048, 2049]
LARGE_P = [524_288, 524_289, 1_100_003]          # 256, 257 and 538 workgroups of 2048 mask bytes: the end of the first turn of
                                                 # k_mask_rank's count loop, its second turn and its third


@pytest.mark.parametrize("P", SMALL_P)
def test_select_rows_small(hip_device, P):
    _check_select(hip_device, P, [4, 12, 16, 36, 180], MASKS, offsets=(0, 5))


@pytest.mark.parametrize("P", LARGE_P)
def test_select_rows_beyond_256_workgroups(hip_device, P):
    _check_select(hip_device, P, [4, 12, 36], MASKS, offsets=(0,))
    _check_select(hip_device, P, [4, 12, 36], ("bernoulli99", "block_ends"), offsets=(5,), seed=1)


def test_select_rows_with_32_tensors(hip_device):
    widths = [4, 12, 16, 36, 180, 8, 24, 60] * 4
    assert len(widths) == 32
    _check_select(hip_device, 2049, widths, ("alternating", "values_0_2_255", "last"), offsets=(5,))


def test_select_rows_appends_behind_the_live_rows_of_the_same_buffer(hip_device):
    """dst is src and dst_row_offset = P, as RowStore.append_selected calls it (clone / split)."""
    dev, P, row_bytes = hip_device, 2049, [4, 12, 180]
    gen = torch.Generator().manual_seed(4)
    for name in ("alternating", "block_ends", "ones", "zeros"):
        mask_cpu = _mask(name, P, gen)
        n = int((mask_cpu != 0).sum())
        live = _source(dev, P, row_bytes)
        bufs, wants = [], []
        for t in live:
            b = torch.full((GUARD + P + n + GUARD, t.shape[1]), SENTINEL, dtype=torch.int32, device=dev)
            b[GUARD:GUARD + P] = t
            wants.append(R.select_ref(t, mask_cpu.to(dev), b, GUARD + P)[0])
            bufs.append(b)
        ptrs = [b[GUARD:].data_ptr() for b in bufs]
        assert _select(dev, P, mask_cpu.to(dev), ptrs, ptrs, row_bytes, P, _dirty_workspace(dev, P)) == n
        for b, w in zip(bufs, wants):
            assert torch.equal(b, w), name


def test_select_rows_second_call_on_a_used_workspace(hip_device):
    """P = 524,289 and then P = 129 on the same workspace: the ranks and workgroup counts of the first call lie where the
    second call's are, and the second result must not depend on them."""
    dev = hip_device
    ws = _dirty_workspace(dev, 524_289)
    gen = torch.Generator().manual_seed(8)
    for P, name in ((524_289, "bernoulli99"), (129, "alternating")):
        mask_cpu = _mask(name, P, gen)
        n = int((mask_cpu != 0).sum())
        src = _source(dev, P, [4, 12, 36])
        sent = [torch.full((GUARD + n + GUARD, t.shape[1]), SENTINEL, dtype=torch.int32, device=dev) for t in src]
        dst = [s.clone() for s in sent]
        got = _select(dev, P, mask_cpu.to(dev), [t.data_ptr() for t in src], [d[GUARD:].data_ptr() for d in dst], [4, 12, 36], 0, ws)
        assert got == n, (P, got, n)
        for t, d, s in zip(src, dst, sent):
            assert torch.equal(d, R.select_ref(t, mask_cpu.to(dev), s, GUARD)[0]), P


@pytest.mark.parametrize("M", [1, 4, 9, 16])
@pytest.mark.parametrize("P", [1, 257, 70_001])
def test_pack_ply_rows_is_save_plys_column_order(hip_device, P, M):
    from luciddreamer_amd import _lib
    dev = hip_device
    gen = torch.Generator().manual_seed(100 * M + P % 97)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dev)
    xyz, f_dc, f_rest, opacity, scaling, rotation = mk(P, 3), mk(P, 1, 3), mk(P, M - 1, 3), mk(P, 1), mk(P, 3), mk(P, 4)
    props = 17 + 3 * (M - 1)
    out = torch.full((GUARD + P * props + GUARD,), float("nan"), device=dev)
    out.view(torch.int32).fill_(SENTINEL)
    want = out.view(torch.int32).clone()
    want[GUARD:GUARD + P * props] = R.pack_ply_ref(xyz, f_dc, f_rest, opacity, scaling, rotation).contiguous().view(torch.int32).view(-1)
    with _lib.on_device(dev):
        rc = _lib.lib().lr_pack_ply_rows(P, M, xyz.data_ptr(), f_dc.data_ptr(), f_rest.data_ptr() if M > 1 else None,
                                         opacity.data_ptr(), scaling.data_ptr(), rotation.data_ptr(), out[GUARD:].data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    assert torch.equal(out.view(torch.int32), want)
