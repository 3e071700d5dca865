"""fused L1 + DSSIM loss and gradient (lr_l1_dssim_forward/backward) vs the CPU oracle
(oracle/loss_oracle.py, float64) and vs the committed outputs of the reference's own functions.
Tolerances (float32 kernel, separable window vs the reference's 2-D window): loss 2e-6 absolute,
gradient 2e-5 of its max."""
import os

import numpy as np
import pytest
import torch

from oracle import loss_oracle

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_loss_fixtures.npz")


def _run(img, gt, lam, dev, upstream=1.0):
    from luciddreamer_amd.loss import l1_dssim_loss
    x = torch.tensor(img, dtype=torch.float32, device=dev, requires_grad=True)
    g = torch.tensor(gt, dtype=torch.float32, device=dev)
    loss = l1_dssim_loss(x, g, lam)
    (loss * upstream).backward()
    return float(loss.item()), x.grad.cpu().numpy()


@pytest.mark.parametrize("case", ("small", "tile_edges", "one_channel", "tiny"))
@pytest.mark.parametrize("lam", (0.2, 1.0, 0.0))
def test_matches_reference_fixture(hip_device, case, lam):
    fx = np.load(FIX)
    loss, grad = _run(fx[f"{case}_img"], fx[f"{case}_gt"], lam, hip_device)
    assert abs(loss - float(fx[f"{case}_lam{lam}_loss"])) <= 2e-6
    ref_g = fx[f"{case}_lam{lam}_grad"]
    assert np.abs(grad - ref_g).max() <= 2e-5 * max(np.abs(ref_g).max(), 1e-12) + 1e-9


@pytest.mark.parametrize("shape", [(3, 256, 256), (3, 97, 131), (3, 1080, 1920)])
def test_matches_oracle(hip_device, shape):
    rng = np.random.default_rng(5)
    gt = rng.random(shape).astype(np.float32)
    img = np.clip(0.6 * gt + 0.4 * rng.random(shape), 0, 1).astype(np.float32)
    big = shape[1] * shape[2] > 1_000_000
    loss, grad = _run(img, gt, 0.2, hip_device, upstream=2.5)
    if big:
        # full 1080p: the oracle's loss only (its autograd gradient of 5 dense 11x11 convolutions takes minutes);
        # the gradient is checked on a window around a corner, an edge and the centre via a cropped oracle run
        o = loss_oracle.l1_dssim(img, gt, 0.2, want_grad=False)
        assert abs(loss - o["loss"]) <= 2e-6
        assert np.isfinite(grad).all()
        C, H, W = shape
        n_full = C * H * W
        for (y0, x0) in ((0, 0), (H - 96, W - 96), (H // 2 - 48, W // 2 - 48), (0, W // 2)):
            crop = (slice(None), slice(y0, y0 + 96), slice(x0, x0 + 96))
            oc = loss_oracle.l1_dssim(img[crop], gt[crop], 0.2)
            # dL/dI(q) depends on pixels within 10 of q: compare where the crop's artificial border cannot reach;
            # the mean's 1/n differs between the crop and the full image
            ref = 2.5 * oc["grad"] * (C * 96 * 96) / n_full
            inner = np.ones((96, 96), bool)
            if y0 > 0: inner[:10] = False
            if y0 + 96 < H: inner[-10:] = False
            if x0 > 0: inner[:, :10] = False
            if x0 + 96 < W: inner[:, -10:] = False
            got = grad[crop]
            assert np.abs(got - ref)[:, inner].max() <= 2e-5 * np.abs(ref).max()
        return
    o = loss_oracle.l1_dssim(img, gt, 0.2)
    assert abs(loss - o["loss"]) <= 2e-6
    ref = 2.5 * o["grad"]
    assert np.abs(grad - ref).max() <= 2e-5 * np.abs(ref).max()


def test_drop_in_names_and_determinism(hip_device):
    from luciddreamer_amd import loss as L
    rng = np.random.default_rng(9)
    a = torch.tensor(rng.random((3, 120, 200)), dtype=torch.float32, device=hip_device)
    b = torch.tensor(rng.random((3, 120, 200)), dtype=torch.float32, device=hip_device)
    o = loss_oracle.l1_dssim(a.cpu().numpy(), b.cpu().numpy(), 0.2, want_grad=False)
    assert abs(L.l1_loss(a, b).item() - o["l1"]) <= 1e-6
    assert abs(L.ssim(a, b).item() - o["ssim"]) <= 2e-6
    assert abs(L.ssim(a, a).item() - 1.0) <= 1e-6
    x = a.clone().requires_grad_(True)
    L.l1_dssim_loss(x, b, 0.2).backward()
    g1 = x.grad.clone()
    x.grad = None
    L.l1_dssim_loss(x, b, 0.2).backward()
    assert torch.equal(g1, x.grad)                         # no atomics: bitwise repeatable
    with pytest.raises(RuntimeError):
        L.l1_dssim_loss(a.cpu(), b.cpu(), 0.2)             # no CPU path
    with pytest.raises(RuntimeError):
        L.l1_dssim_loss(a, b[:, :-1], 0.2)


def test_terms_share_the_size_cache_and_the_call_path(hip_device):
    """Every loss term, forward and backward, at two shapes in one process, shapes and terms alternating and the whole tour made
    twice: each entry of the shared workspace-size cache is made by one visit and read by the next after five other terms have
    gone through the same cache and call helper.  16x16 is one workgroup everywhere and smaller than the 32-pixel SSIM tile;
    47x61 crosses the tile edge in both axes and the 2048-pixel workgroup of the plane kernels.  Each first visit is held to the
    reference and the bar of the term's own test (this file, test_gpu_depth_views.py, test_gpu_depth_pearson.py,
    test_gpu_mask_views.py), with that test's upstream scalar (the plane terms' gradients are compared with torch's bit for bit:
    torch divides by H*W through the reciprocal, which rounds as the kernels' division does for 1.3 * 0.7 at these sizes);
    each second visit returns the first one's bits."""
    from luciddreamer_amd import _lib, loss as L
    from tests import depth_l1_ref, depth_pearson_ref, mask_loss_ref
    dev, lam, up, up_plane = hip_device, 0.2, 2.5, 1.3
    data, want = {}, {}
    for H, W in ((16, 16), (47, 61)):
        rng = np.random.default_rng(H + W)
        gt = rng.random((3, H, W)).astype(np.float32)
        img = np.clip(0.6 * gt + 0.4 * rng.random((3, H, W)), 0, 1).astype(np.float32)
        m = mask_loss_ref.make_mask(H, W, seed=H * 3 + W, kind="soft")
        d, t = depth_l1_ref.make_pair(H, W, seed=H + W, lead=(1,))
        alpha = torch.rand(1, H, W, generator=torch.Generator().manual_seed(H + W))
        data[H, W] = {k: torch.as_tensor(v).to(dev) for k, v in dict(img=img, gt=gt, m=m, d=d, t=t, alpha=alpha).items()}
        want[H, W] = dict(pair=loss_oracle.l1_dssim(img, gt, lam), masked=mask_loss_ref.numpy_masked_l1_dssim(img, gt, m.numpy(), lam),
                          depth_l1=depth_l1_ref.numpy_depth_l1(d.numpy(), t.numpy(), 0.7)[0],
                          pearson=depth_pearson_ref.numpy_depth_pearson(d.numpy(), t.numpy(), 0.7),
                          alpha=mask_loss_ref.numpy_alpha_hole(alpha.numpy(), m.numpy(), 0.7)[0])
    paired = L.PairedLoss()

    def visit(term, D, image=None, lead=()):
        """(value[s], gradient) of one forward + backward; image: the leaf to use in place of a fresh contiguous [C,H,W] one;
        lead: leading dims of the image pair."""
        leaf = {"depth_l1": "d", "depth_pearson": "d", "alpha_hole": "alpha"}.get(term, "img")
        x = (D[leaf].clone() if image is None else image).requires_grad_(True)
        gt = D["gt"].reshape(*lead, *D["gt"].shape)
        if term == "l1_dssim_loss":
            vals = (L.l1_dssim_loss(x, gt, lam),)
        elif term == "paired":
            vals = (paired.l1_loss(x, D["gt"]), paired.ssim(x, D["gt"]))
        elif term == "masked_l1_dssim":
            vals = (L.masked_l1_dssim(x, gt, D["m"], lam),)
        elif term == "depth_l1":
            vals = (L.depth_l1(x, D["t"], 0.7),)
        elif term == "depth_pearson":
            vals = (L.depth_pearson(x, D["t"], 0.7),)
        else:
            vals = (L.alpha_hole(x, D["m"], 0.7),)
        total = vals[0] if len(vals) == 1 else (1.0 - lam) * vals[0] + lam * (1.0 - vals[1])
        (total * (up if leaf == "img" else up_plane)).backward()
        return tuple(v.detach().clone() for v in vals), x.grad

    terms = ("l1_dssim_loss", "paired", "masked_l1_dssim", "depth_l1", "depth_pearson", "alpha_hole")
    tours = [{(term, hw): visit(term, data[hw]) for hw in data for term in terms} for _ in range(2)]
    for key, (vals, grad) in tours[0].items():
        again = tours[1][key]
        assert all(torch.equal(a, b) for a, b in zip(vals, again[0])) and torch.equal(grad, again[1]), key
    for hw, D in data.items():
        first = lambda term: tours[0][term, hw]
        o = want[hw]["pair"]
        (loss,), grad = first("l1_dssim_loss")
        print(f"[terms] {hw} l1_dssim_loss {float(loss):.8f} want {o['loss']:.8f}")
        assert abs(float(loss) - o["loss"]) <= 2e-6
        assert np.abs(grad.cpu().numpy() - up * o["grad"]).max() <= 2e-5 * np.abs(up * o["grad"]).max()
        (l1, ss), grad = first("paired")
        assert abs(float(l1) - o["l1"]) <= 1e-6 and abs(float(ss) - o["ssim"]) <= 2e-6
        assert np.abs(grad.cpu().numpy() - up * o["grad"]).max() <= 2e-5 * np.abs(up * o["grad"]).max()
        o = want[hw]["masked"]
        (loss,), grad = first("masked_l1_dssim")
        assert abs(float(loss) - o["loss"]) <= 2e-6
        assert np.abs(grad.cpu().numpy() - up * o["grad"]).max() <= 2e-5 * np.abs(up * o["grad"]).max()
        (loss,), grad = first("depth_l1")
        assert abs(float(loss) - want[hw]["depth_l1"]) <= 1e-6 * abs(want[hw]["depth_l1"])
        ref = D["d"].clone().requires_grad_(True)
        (depth_l1_ref.torch_depth_l1(ref, D["t"], 0.7) * up_plane).backward()
        assert torch.equal(grad, ref.grad) and float(grad.abs().max()) > 0
        w_loss, _, w_grad = want[hw]["pearson"]
        (loss,), grad = first("depth_pearson")
        assert abs(float(loss) - w_loss) <= 1e-6
        assert np.abs(w_grad).max() > 0 and np.abs(grad.cpu().numpy() - up_plane * w_grad).max() <= 1e-6 * up_plane * np.abs(w_grad).max()
        (loss,), grad = first("alpha_hole")
        assert abs(float(loss) - want[hw]["alpha"]) <= 1e-6 * abs(want[hw]["alpha"])
        ref = D["alpha"].clone().requires_grad_(True)
        (mask_loss_ref.torch_alpha_hole(ref, D["m"], 0.7) * up_plane).backward()
        assert torch.equal(grad, ref.grad) and float(grad.abs().max()) > 0
        # the image terms once more through the wrapper's own copy: a transposed view (not contiguous) and [1,C,H,W]
        for term in ("l1_dssim_loss", "paired", "masked_l1_dssim"):
            vals, grad = first(term)
            view = D["img"].transpose(1, 2).contiguous().transpose(1, 2)
            assert not view.is_contiguous()
            v2, g2 = visit(term, D, view)
            assert all(torch.equal(a, b) for a, b in zip(vals, v2)) and torch.equal(grad, g2), (term, hw, "view")
            if term != "paired":                                           # the shared pass of the pair takes [C,H,W] only
                v4, g4 = visit(term, D, D["img"][None].clone(), lead=(1,))
                assert all(torch.equal(a, b) for a, b in zip(vals, v4)) and tuple(g4.shape) == (1, 3, *hw), (term, hw)
                assert torch.equal(grad, g4[0])
    # one cache, one entry per size query and shape, holding the library's answer
    lib = _lib.lib()
    for H, W in data:
        assert L._WS_BYTES["lr_loss_workspace_bytes", (3, H, W)] == lib.lr_loss_workspace_bytes(3, H, W)
        for q in ("lr_depth_l1_workspace_bytes", "lr_depth_pearson_workspace_bytes", "lr_alpha_hole_workspace_bytes"):
            assert L._WS_BYTES[q, (H, W)] == getattr(lib, q)(H, W) > 0


def test_training_step_matches_torch_composition(hip_device):
    """render -> fused loss -> backward gives the same parameter gradients as render -> torch L1/SSIM composition."""
    import torch.nn.functional as F
    from luciddreamer_amd import cameras, synthetic
    from luciddreamer_amd.gaussian_renderer import GaussianCloud, render_raw
    from luciddreamer_amd.loss import l1_dssim_loss
    dev = hip_device
    W, H, P = 256, 192, 4000
    cloud = {k: v.to(dev) for k, v in synthetic.make_cloud(P, "box", 3).items()}
    pc = GaussianCloud(cloud["means3D"], cloud["scales"], cloud["rotations"], cloud["opacities"], cloud["shs"])
    cam = cameras.identity_camera(W, H).to(dev)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)

    def torch_loss(img):
        w1 = loss_oracle.window_1d().to(dev).unsqueeze(1)
        win = (w1 @ w1.t()).expand(3, 1, 11, 11).contiguous()
        conv = lambda t: F.conv2d(t[None], win, padding=5, groups=3)[0]
        mu1, mu2 = conv(img), conv(gt)
        s1, s2, s12 = conv(img * img) - mu1 * mu1, conv(gt * gt) - mu2 * mu2, conv(img * gt) - mu1 * mu2
        m = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))
        return 0.8 * (img - gt).abs().mean() + 0.2 * (1 - m.mean())

    grads = []
    for fn in (lambda im: l1_dssim_loss(im, gt, 0.2), torch_loss):
        for p in pc.parameters():
            p.grad = None
        fn(render_raw(cam, pc)["render"]).backward()
        grads.append([p.grad.clone() for p in pc.parameters()])
    for a, b in zip(*grads):
        assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item() + 1e-12
