"""CPU: every argument check that sits in front of the first HIP call of the loss entry points other than the Pearson pair
(tests/test_depth_pearson_cpu.py has those): lr_l1_dssim_*, lr_masked_l1_dssim_*, lr_depth_l1_* and lr_alpha_hole_*.  One table
row per entry point: its arguments in order, its required pointers, its dims and the message of each refusal.  Every pointer
is one small host buffer; no case gets as far as a launch.

`upstream` is NULL in every case and `weight` is negative or NaN in some, and each case still names another fault: neither
is refused here (only the Pearson pair checks its weight).  The forwards show it with a fault that comes last in the order
of checks, the workspace bound; the backwards without a workspace size have no later check to show it by."""
import ctypes

import pytest

IMAGE_DIMS = b"channels, height, width must be positive"
PLANE_DIMS = b"height, width must be positive (and H*W < 2^31)"
IMAGE, PLANE = ("C", "H", "W"), ("H", "W")

# entry point -> (arguments in order, dims, required pointers, their message, (size query, its message) or None)
ENTRY = {
    "lr_l1_dssim_forward": (("C", "H", "W", "image", "gt", "lam", "out", "ws", "ws_bytes", "stream"), IMAGE,
                            ("image", "gt", "out", "ws"), b"image/gt/out_loss3/workspace are required",
                            ("lr_loss_workspace_bytes", b"loss workspace too small (lr_loss_workspace_bytes)")),
    "lr_l1_dssim_backward": (("C", "H", "W", "image", "gt", "lam", "upstream", "ws", "grad", "stream"), IMAGE,
                             ("image", "gt", "ws", "grad"), b"image/gt/workspace/dL_dimage are required", None),
    "lr_l1_dssim_backward_weights": (("C", "H", "W", "image", "gt", "w_l1", "w_ssim", "ws", "grad", "stream"), IMAGE,
                                     ("image", "gt", "ws", "grad", "w_l1", "w_ssim"),
                                     b"image/gt/workspace/dL_dimage/w_l1/w_ssim are required", None),
    "lr_masked_l1_dssim_forward": (("C", "H", "W", "image", "gt", "mask", "lam", "out", "ws", "ws_bytes", "stream"), IMAGE,
                                   ("image", "gt", "mask", "out", "ws"), b"image/gt/mask/out_loss3/workspace are required",
                                   ("lr_loss_workspace_bytes", b"loss workspace too small (lr_loss_workspace_bytes)")),
    "lr_masked_l1_dssim_backward": (("C", "H", "W", "image", "gt", "mask", "lam", "upstream", "ws", "grad", "stream"), IMAGE,
                                    ("image", "gt", "mask", "ws", "grad"), b"image/gt/mask/workspace/dL_dimage are required", None),
    "lr_depth_l1_forward": (("H", "W", "depth", "target", "weight", "out", "ws", "ws_bytes", "stream"), PLANE,
                            ("depth", "target", "out", "ws"), b"depth/target/out_loss/workspace are required",
                            ("lr_depth_l1_workspace_bytes", b"depth loss workspace too small (lr_depth_l1_workspace_bytes)")),
    "lr_depth_l1_backward": (("H", "W", "depth", "target", "weight", "upstream", "grad", "stream"), PLANE,
                             ("depth", "target", "grad"), b"depth/target/dL_ddepth are required", None),
    "lr_alpha_hole_forward": (("H", "W", "alpha", "mask", "weight", "out", "ws", "ws_bytes", "stream"), PLANE,
                              ("alpha", "mask", "out", "ws"), b"alpha/mask/out_loss/workspace are required",
                              ("lr_alpha_hole_workspace_bytes", b"alpha hole workspace too small (lr_alpha_hole_workspace_bytes)")),
    "lr_alpha_hole_backward": (("H", "W", "mask", "weight", "upstream", "grad", "stream"), PLANE,
                               ("mask", "grad"), b"mask/dL_dalpha are required", None),
}
BAD_WEIGHTS = (-0.5, float("nan"), float("inf"))


def _cases():
    """(entry point, case name, overrides of a valid call, message fragment)."""
    out = []
    for name, (order, dims, required, ptr_msg, query) in ENTRY.items():
        dims_msg = IMAGE_DIMS if dims is IMAGE else PLANE_DIMS
        for p in required:
            out.append((name, "null_" + p, {p: None}, ptr_msg))
        for d in dims:
            out.append((name, "zero_" + d, {d: 0}, dims_msg))
            out.append((name, "negative_" + d, {d: -3}, dims_msg))
        if dims is PLANE:
            out.append((name, "too_many_pixels", dict(H=65536, W=65536), dims_msg))
        # the order of the checks: dims in front of pointers, pointers in front of the workspace bound
        out.append((name, "dims_before_pointers", {dims[-1]: 0, required[0]: None}, dims_msg))
        if query:
            out.append((name, "workspace_one_byte_short", dict(ws_bytes=-1), query[1]))
            out.append((name, "workspace_zero", dict(ws_bytes=0), query[1]))
            out.append((name, "pointers_before_workspace", dict(ws_bytes=-1, out=None), ptr_msg))
            for w in BAD_WEIGHTS if "weight" in order else ():
                out.append((name, f"weight_{w}_is_not_refused", dict(weight=w, ws_bytes=-1), query[1]))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


def test_the_table_covers_the_entry_points_with_their_prototypes(L):
    from luciddreamer_amd import _lib
    for name, (order, dims, required, _, query) in ENTRY.items():
        assert name in _lib.EXPORTS and len(getattr(L, name).argtypes) == len(order), name
        assert set(required) <= set(order) and set(dims) <= set(order) and "upstream" not in required
        assert (query is not None) == ("ws_bytes" in order)
    assert len({(n, c) for n, c, _, _ in CASES}) == len(CASES)


@pytest.mark.parametrize("name,case,over,fragment", CASES, ids=[f"{n}-{c}" for n, c, _, _ in CASES])
def test_argument_checks_without_a_device(L, name, case, over, fragment):
    from luciddreamer_amd import _lib
    order, dims, _, _, query = ENTRY[name]
    buf = (ctypes.c_float * 64)()                                         # 256 bytes stand in for every pointer
    p = ctypes.addressof(buf)
    a = dict.fromkeys(order, p)
    a.update(C=3, H=16, W=16, lam=0.2, weight=1.0, upstream=None, stream=None, ws_bytes=1 << 20)
    a.update(over)
    if a["ws_bytes"] == -1:                                               # one byte short of the size query, for the call's dims
        n = getattr(L, query[0])(*(a[d] for d in dims))
        assert n > 0
        a["ws_bytes"] = n - 1
    rc = getattr(L, name)(*(a[k] for k in order))
    assert rc == _lib.LR_ERR_INVALID_ARG
    assert fragment in L.lr_last_error(), L.lr_last_error()
