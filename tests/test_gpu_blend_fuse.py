"""GPU: the blend forward and backward of a step's view in ONE launch (render_bwd.hip k_render_bwd_tile_step;
lr_tune_set("blend_fuse", 2): every view that qualifies) against the two launches it replaces ("blend_fuse" 0: k_render_fwd_tile,
colour-free, then k_render_bwd_tile, which the parity tests hold to the oracle), inside one build and BYTE FOR BYTE -- the fused
kernel runs the text of the two kernels in the same order, so there is no tolerance.  Both runs are forced to the
one-wave-per-tile shapes ("fwd_pair" 2, "blend_quad" 2): the other shapes round the backward's sums in another order.

Every case runs lr_views_accumulate with fixed dL_dpix under both knob values on a zeroed workspace and compares every
accumulator (dL_dmean2D among them) and, in every workspace slot, the 64 header words, final_T, n_contrib, the forward's quadrant
tests and the per-instance gradient slots.  That the knob took the path it names is read from the stage records: a fused view
records no render_fwd call.

Scenes: 50 x 37 (partial tiles on both edges) and 48 x 32; one tile of EXACTLY n entries around the backward's round of 30, the
forward's of 64 and one, two and three segments of 256, stacked so that its centre pixels stop early and the others never; beside
it forty opaque layers over one quadrant of another tile (that quadrant finishes before the others) with splats behind them, whose
rectangles reach the edge tiles, and tiles no Gaussian reaches; a view whose binning capacity is too small; strict mode; four views on three
chains, run twice; a view whose colour the caller keeps inside a step of views that qualify."""
import numpy as np
import pytest
import torch

from luciddreamer_amd import _lib, cameras
from tests import helpers as hp
from tests.test_gpu_bin_fuse import _splats
from tests.test_gpu_step_invariants import ACC_SHAPES, _bits_equal, _host_array, _scene as _step_scene

pytestmark = pytest.mark.gpu

CAPACITY = 8192
SIZES = [0, 1, 30, 31, 60, 64, 65, 128, 256, 257, 600]


@pytest.fixture(autouse=True)
def _knobs():
    _lib.tune_set("fwd_pair", 2)
    _lib.tune_set("blend_quad", 2)
    yield
    for k in ("blend_fuse", "fwd_pair", "blend_quad", "strict"):
        _lib.tune_set(k, -1)


def _align(n):
    return (n + 255) // 256 * 256


def _slots(batch, P, w, h, capacity, n_slots):
    """What the blend pair left in every workspace slot (csrc/common.h geom / img / bin layouts, api.hip view_slot_layout)."""
    L = _lib.lib()
    ws = batch.workspace.cpu().numpy()
    slot_bytes = int(L.lr_views_workspace_bytes(P, w, h, capacity, 2, 0)) - int(L.lr_views_workspace_bytes(P, w, h, capacity, 1, 0))
    geom_bytes, img_bytes = int(L.lr_geom_bytes(P)), int(L.lr_img_bytes(w, h))
    N = w * h
    out = []
    for i in range(n_slots):
        s = ws[i * slot_bytes:(i + 1) * slot_bytes]
        hdr = s[:256].view(np.uint32).copy()
        overflow, n_sorted = int(hdr[1]), int(hdr[5])
        img = s[geom_bytes:geom_bytes + img_bytes]
        b = s[geom_bytes + img_bytes:]
        quad_off = _align(4 * capacity)
        grad_off = quad_off + _align(8 * capacity) + _align(4 * capacity)
        d = dict(hdr=hdr, final_T=img[:4 * N].view(np.uint32).copy(),
                 n_contrib=img[_align(4 * N):_align(4 * N) + 4 * N].view(np.uint32).copy(),
                 quad_hits=b[quad_off:quad_off + 4 * n_sorted].view(np.uint32).copy())
        if not overflow:                                    # (an overflowed view is not differentiated: its slots are never written)
            d["inst_grad"] = b[grad_off:grad_off + 48 * n_sorted].view(np.uint32).copy()
        out.append(d)
    return out


def _step(device, cloud, cams, grads, *, capacity=CAPACITY, n_streams=3, keep_color=()):
    """One step on a zeroed workspace; returns the accumulators, what the slots hold, the kept colour images and the number of
    blend-forward launches the step recorded."""
    from luciddreamer_amd import parallel
    P = cloud["means3D"].shape[0]
    w, h = cams[0].image_width, cams[0].image_height
    batch = parallel.ViewBatch(cams, grads, 3, torch.tensor([0.1, 0.0, 0.2], device=device), binning_capacity=capacity,
                               n_streams=n_streams)
    colors = [torch.full((3, h, w), -1.0, device=device) if v in keep_color else None for v in range(len(cams))]
    if keep_color:
        batch._args.out_color = _host_array(batch, colors)
    batch.use_workspace(torch.zeros((batch.workspace_bytes(P),), dtype=torch.uint8, device=device), P)
    acc = {k: torch.zeros((P,) + s, device=device) for k, s in ACC_SHAPES.items()}
    _lib.profile_enable(True)
    batch.run(cloud["means3D"], cloud["opacities"], cloud["scales"], cloud["rotations"], cloud["shs"], acc)
    torch.cuda.synchronize()
    fwd_calls = _lib.profile_read()["render_fwd"][1]
    _lib.profile_enable(False)
    return dict(acc=acc, slots=_slots(batch, P, w, h, capacity, min(n_streams, len(cams))),
                color=[c for c in colors if c is not None], fwd_calls=fwd_calls)


def _assert_same_step(got, want, what):
    for k in want["acc"]:
        assert _bits_equal(got["acc"][k], want["acc"][k]), (what, k)
    assert len(got["slots"]) == len(want["slots"])
    for i, (a, b) in enumerate(zip(got["slots"], want["slots"])):
        assert a.keys() == b.keys(), (what, i)
        for k in b:
            assert np.array_equal(a[k], b[k]), (what, "slot", i, k)
    assert len(got["color"]) == len(want["color"])
    for a, b in zip(got["color"], want["color"]):
        assert _bits_equal(a, b), (what, "color")


def _pair(device, cloud, cams, grads, n_fused=None, **kw):
    """The step under blend_fuse 0 and 2: the same bytes, and each knob on the path it names."""
    n_views = len(cams)
    n_fused = n_views if n_fused is None else n_fused
    _lib.tune_set("blend_fuse", 0)
    want = _step(device, cloud, cams, grads, **kw)
    assert want["fwd_calls"] == n_views
    _lib.tune_set("blend_fuse", 2)
    got = _step(device, cloud, cams, grads, **kw)
    assert got["fwd_calls"] == n_views - n_fused
    assert _lib.last_launch_shapes() == ("tile", "tile")
    _assert_same_step(got, want, "blend_fuse 2 against 0")
    return want


def _stacked_scene(cam, n, w, h, seed):
    """Tile A = gx (the left tile of the second row, pixels 0..15 x 16..31) holds exactly n small splats of opacity 0.9 stacked on
    the 7 x 7 pixels around its centre: a pixel under five of them stops early, the tile's corners are never touched, and the four
    quadrants see different subsets.  Tile B = gx + 2 (pixels 32..47 x 16..31): forty opaque layers of sigma = 4 pixels centred on
    its upper left quadrant, in front of sixty small splats -- every pixel of that quadrant stops within the first round of 64, the
    far corner of the tile never.  The layers' rectangles (13 pixels each way) also reach the tiles right of and below B, the
    partial ones of a 50 x 37 image among them; seven small splats on each of tiles 1 and 2; the tiles of the left column other
    than A are reached by nothing."""
    gx = (w + 15) // 16
    rng = np.random.default_rng(seed)
    tile_of = np.concatenate([np.full(n, gx), np.full(60, gx + 2), np.full(7, 1), np.full(7, 2)])
    depth = rng.permutation(np.linspace(2.0, 6.0, tile_of.shape[0], dtype=np.float32)).astype(np.float32)
    cloud = _splats(cam, tile_of, depth, w, h, seed=seed)
    # the opaque layers: view depth 1.0 .. 1.4, sigma 4 pixels, centred on pixel (35.5, 19.5)
    tfx, tfy = hp.tan_fov(cam)
    n_big = 40
    z = np.linspace(1.0, 1.4, n_big)
    means = np.stack([((2 * 35.5 + 1) / w - 1) * z * tfx, ((2 * 19.5 + 1) / h - 1) * z * tfy, z], axis=1).astype(np.float32)
    scale = (4.0 * 2.0 * tfx * z / w).astype(np.float32)
    shs = torch.zeros(n_big, 16, 3)
    shs[:, 0, :] = torch.from_numpy(rng.random((n_big, 3)).astype(np.float32))
    rot = torch.zeros(n_big, 4)
    rot[:, 0] = 1.0
    big = dict(means3D=torch.from_numpy(means), scales=torch.from_numpy(scale)[:, None].repeat(1, 3), rotations=rot,
               opacities=torch.full((n_big, 1), 0.99), shs=shs)
    return {k: torch.cat([cloud[k], big[k]]).contiguous() for k in cloud}


def _grads(w, h, n, device, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(3, h, w, generator=g).to(device) for _ in range(n)]


# ---- 1. one tile of exactly n entries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(50, 37), (48, 32)])
@pytest.mark.parametrize("n", SIZES)
def test_one_tile_of_exactly_n(hip_device, n, size):
    w, h = size
    cam = cameras.identity_camera(w, h)
    cloud = {k: v.to(hip_device) for k, v in _stacked_scene(cam, n, w, h, seed=100 + n).items()}
    want = _pair(hip_device, cloud, [cam.to(hip_device)], _grads(w, h, 1, hip_device), n_streams=1)
    s = want["slots"][0]
    # the scene is what it says (n_contrib: the position that stopped the pixel, or the list's length)
    last = s["n_contrib"].reshape(h, w)
    tile_a, tile_b = last[16:32, 0:16], last[16:32, 32:48]
    assert int(tile_a.max()) == n                                   # the tile's list, and a pixel that never stopped
    if n >= 256:
        assert int(tile_a.min()) < n                                # six or more splats on one pixel (49 positions): it stopped early
    total_b = int(tile_b.max())
    assert total_b == 100 and int(tile_b[15, 15]) == 100            # forty layers and sixty splats; the far corner never stops
    assert int(tile_b[0:8, 0:8].max()) < 64                         # the quadrant under the layers: finished in the first round
    assert int(s["hdr"][1]) == 0 and int(s["hdr"][10]) == 0         # no overflow, nothing left uncovered
    assert int(s["hdr"][9]) == (max(n, 1) - 1) // 256               # n_seg: tile A's segments beyond the first
    assert float(want["acc"]["means3D"].abs().max()) > 0


# ---- 2. overflow ---------------------------------------------------------------------------------------------------------------
def test_overflowed_view_has_no_gradient_under_either_knob(hip_device):
    w, h = 50, 37
    cam = cameras.identity_camera(w, h)
    cloud = {k: v.to(hip_device) for k, v in _stacked_scene(cam, 128, w, h, seed=7).items()}
    want = _pair(hip_device, cloud, [cam.to(hip_device)], _grads(w, h, 1, hip_device), n_streams=1, capacity=300)
    s = want["slots"][0]
    assert int(s["hdr"][1]) == 1 and int(s["hdr"][5]) == 300 and "inst_grad" not in s
    for k, t in want["acc"].items():
        assert float(t.abs().max()) == 0.0, k


# ---- 3. strict mode ------------------------------------------------------------------------------------------------------------
def test_strict_mode(hip_device):
    w, h = 50, 37
    cam = cameras.identity_camera(w, h)
    cloud = {k: v.to(hip_device) for k, v in _stacked_scene(cam, 257, w, h, seed=9).items()}
    _lib.tune_set("strict", 1)
    want = _pair(hip_device, cloud, [cam.to(hip_device)], _grads(w, h, 1, hip_device), n_streams=1)
    assert float(want["acc"]["means3D"].abs().max()) > 0


# ---- 4. four views on three chains, twice --------------------------------------------------------------------------------------
def test_four_views_on_three_chains_twice(hip_device):
    sc = _step_scene(hip_device, "band")
    cams = sc["cams"][:4]
    grads = [sc["grad"]] * 4
    want = _pair(hip_device, sc["cloud"], cams, grads, n_streams=3, capacity=200_000)
    for knob in (2, 0, 2):
        _lib.tune_set("blend_fuse", knob)
        _assert_same_step(_step(hip_device, sc["cloud"], cams, grads, n_streams=3, capacity=200_000), want, f"again, blend_fuse {knob}")
    assert float(want["acc"]["means3D"].abs().max()) > 0


# ---- 5. a view that does not qualify inside a step of views that do ------------------------------------------------------------
def test_view_whose_colour_is_kept_takes_the_two_launches(hip_device):
    sc = _step_scene(hip_device, "band")
    cams = sc["cams"][:4]
    grads = [sc["grad"]] * 4
    want = _pair(hip_device, sc["cloud"], cams, grads, n_fused=3, n_streams=3, capacity=200_000, keep_color=(1,))
    assert len(want["color"]) == 1 and float(want["color"][0].min()) >= 0      # written, by the unfused forward
    assert _lib.last_forward_channels() == "none"                               # the step's last view: the colour-free blend


# ---- 6. the knob ---------------------------------------------------------------------------------------------------------------
def test_knob_values(hip_device):
    for v in (-1, 0, 1, 2):
        _lib.tune_set("blend_fuse", v)
    for v in (-2, 3):
        with pytest.raises(RuntimeError):
            _lib.tune_set("blend_fuse", v)
