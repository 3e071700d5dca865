"""References of the mask supervision losses (luciddreamer_amd.loss.masked_l1_dssim / alpha_hole, and the fused multi-view step
lr_views_accumulate with masks):

    Lc = l1_dssim(m * I, m * G, lambda)          dLc/dI = m * (d l1_dssim / dI')|_{I' = m I}
    La = weight * mean_{H*W}( A * (1 - m) )      dLa/dA = weight * (1 - m) / (H*W)

`torch_*` are those definitions in torch (autograd gives the gradients); `numpy_*` restate them in float64: Lc from
oracle.loss_oracle.l1_dssim on the masked pair with its gradient multiplied by m, La and its gradient in closed form.
`make_mask` draws the two kinds of masks the tests use: soft random values in [0, 1], and a LucidDreamer-like binary mask (a
scatter of projected points, dilated then eroded, with large holes)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss_oracle


def torch_masked_l1_dssim(image, gt, mask, lam=0.2):
    """image, gt [C,H,W], mask [1,H,W] or [H,W]; the reference composition (l1 + ssim of oracle.loss_oracle) on the masked pair."""
    m = mask.reshape(1, *image.shape[-2:])
    x, g = image * m, gt * m
    l1 = (x - g).abs().mean()
    s = loss_oracle.ssim_map(x, g).mean()
    return (1.0 - lam) * l1 + lam * (1.0 - s)


def numpy_masked_l1_dssim(image, gt, mask, lam=0.2, want_grad=True):
    """dict(loss, l1, ssim[, grad]) in float64."""
    m = np.asarray(mask, dtype=np.float64).reshape(1, *np.shape(image)[-2:])
    o = loss_oracle.l1_dssim(np.asarray(image, np.float64) * m, np.asarray(gt, np.float64) * m, lam, want_grad=want_grad)
    if want_grad:
        o["grad"] = o["grad"] * m
    return o


def torch_alpha_hole(alpha, mask, weight=1.0):
    return weight * (alpha * (1 - mask.reshape(alpha.shape))).mean()


def numpy_alpha_hole(alpha, mask, weight=1.0):
    """(loss, dloss/dalpha) in float64."""
    a = np.asarray(alpha, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64).reshape(a.shape)
    return float(weight * (a * (1 - m)).sum() / a.size), weight * (1 - m) / a.size


def make_mask(H, W, seed, kind="binary"):
    """float32 [1,H,W]: "soft" uniform values in [0, 1] (a fifth of them exact 0 or 1); "binary" a LucidDreamer-like content mask."""
    g = torch.Generator().manual_seed(seed)
    if kind == "soft":
        m = torch.rand(1, H, W, generator=g)
        u = torch.rand(1, H, W, generator=g)
        m = torch.where(u < 0.1, torch.zeros_like(m), torch.where(u < 0.2, torch.ones_like(m), m))
        return m.contiguous()
    # points scattered with a density that falls off to one side, dilated (radius 2) then eroded (radius 1): a ragged cover
    dens = torch.linspace(0.6, 0.05, W).expand(H, W)
    pts = (torch.rand(H, W, generator=g) < dens).float()[None, None]
    dil = F.max_pool2d(pts, 5, 1, 2)
    ero = -F.max_pool2d(-dil, 3, 1, 1)
    m = ero[0]
    # large holes: two rectangles of no content
    for _ in range(2):
        h, w = max(1, H // 4), max(1, W // 5)
        y0 = int(torch.randint(0, max(1, H - h), (1,), generator=g))
        x0 = int(torch.randint(0, max(1, W - w), (1,), generator=g))
        m[:, y0:y0 + h, x0:x0 + w] = 0
    return m.contiguous()
