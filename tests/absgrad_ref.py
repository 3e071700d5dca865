"""Float64 reference of the absgrad output (test helper, not collected).

lr_view_backward with dL_dmean2D_abs returns, per Gaussian i, (sum_p |g[p,i].x|, sum_p |g[p,i].y|, 0): g[p,i] the part of dL/dmeans2D_i[:2] that
flows through pixel p, in the NDC scale of dL_dmean2D.  tests/grad_oracle.render takes means2D as a virtual screen-space offset
in NDC units, so the gradient of a scalar with respect to it IS dL_dmean2D; here every pixel's share of L is back-propagated on
its own (one autograd.grad per pixel) and the magnitudes are summed.  The signed sum of the same per-pixel gradients is returned
too: it must be the whole-image gradient, which is how the reference checks itself (tests/test_absgrad_cpu.py)."""
import functools

import numpy as np
import torch

from tests import absgrad_cases as cases
from tests import grad_oracle

LEAVES = ("means2D", "opacity", "means3D", "sh", "scales", "rotations")


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict: abs, signed (P,2) float64 numpy; grads {leaf: float64 numpy} of the whole-image L; radii (P,) int32; layers
    (grad_oracle's per-tile dicts).  Computed once per process and case; callers do not modify it."""
    case = cases.make(name)
    if name == "partial_strict":                        # strict mode evaluates the same function
        return reference("partial")
    cam, cloud = case["cam"], cases.reference_cloud(case)
    tfx, tfy = cases.tan_fov(cam)
    H, W = cam.image_height, cam.image_width
    d = lambda t: t.detach().to(torch.float64).requires_grad_(True)
    leaves = dict(means3D=d(cloud["means3D"]), opacity=d(cloud["opacities"]), scales=d(cloud["scales"]),
                  rotations=d(cloud["rotations"]), sh=d(cloud["shs"]))
    P = leaves["means3D"].shape[0]
    leaves["means2D"] = torch.zeros(P, 3, dtype=torch.float64, requires_grad=True)
    color, depth, alpha, radii, layers = grad_oracle.render(
        leaves["means3D"], leaves["opacity"], cam.world_view_transform, cam.full_proj_transform, cam.camera_center, tfx, tfy,
        H, W, case["bg"], scales=leaves["scales"], rotations=leaves["rotations"], shs=leaves["sh"], degree=cases.DEGREE,
        means2D=leaves["means2D"], alpha=True, with_layers=True)
    per_pixel = (color * case["g_color"].to(torch.float64)).sum(0)              # (H, W): every pixel's share of L
    if case["g_depth"] is not None:
        per_pixel = per_pixel + (depth * case["g_depth"].to(torch.float64))[0]
    if case["g_alpha"] is not None:
        per_pixel = per_pixel + (alpha * case["g_alpha"].to(torch.float64))[0]
    flat = per_pixel.reshape(-1)
    abs_sum = torch.zeros(P, 2, dtype=torch.float64)
    signed = torch.zeros(P, 2, dtype=torch.float64)
    for k in range(flat.numel()):
        (g,) = torch.autograd.grad(flat[k], leaves["means2D"], retain_graph=True)
        abs_sum += g[:, :2].abs()
        signed += g[:, :2]
    whole = torch.autograd.grad(flat.sum(), [leaves[k] for k in LEAVES], allow_unused=True)
    grads = {k: (np.zeros(tuple(leaves[k].shape)) if g is None else g.numpy()) for k, g in zip(LEAVES, whole)}
    return dict(abs=abs_sum.numpy(), signed=signed.numpy(), grads=grads, radii=radii.numpy(), layers=layers, n_pixels=H * W)


@functools.lru_cache(maxsize=None)
def fragile_rows(name):
    """(rows, visible): indices of the Gaussians that touch a pixel the CPU oracle flags as sitting within rounding of a
    discrete threshold (alpha = 1/255, T = 1e-4; helpers.compare_grads_by_row's test of "touches"), and the number of visible
    rows.  The GPU test may leave these rows out of the comparison, within cases.FRAGILE_ROW_CAP of the visible rows."""
    from oracle import oracle
    case = cases.make(name)
    cam, cloud = case["cam"], cases.reference_cloud(case)
    tfx, tfy = cases.tan_fov(cam)
    n = lambda t: t.detach().cpu().numpy()
    res = oracle.forward(n(case["bg"]), n(cloud["means3D"]), None, n(cloud["opacities"]), n(cloud["scales"]), n(cloud["rotations"]),
                         1.0, None, n(cam.world_view_transform), n(cam.full_proj_transform), tfx, tfy, cam.image_height,
                         cam.image_width, n(cloud["shs"]), cases.DEGREE, n(cam.camera_center), False)
    st = res.stage()
    fy, fx = np.nonzero(st["fragile"] != 0)
    visible = np.nonzero(res.radii > 0)[0]
    rows = []
    for i in visible:
        ca, cb, cc, op = st["conic_opacity"][i].astype(np.float64)
        dx, dy = st["means2D"][i, 0] - fx.astype(np.float64), st["means2D"][i, 1] - fy.astype(np.float64)
        power = -0.5 * (ca * dx * dx + cc * dy * dy) - cb * dx * dy
        if ((power <= 1e-6) & (op * np.exp(np.minimum(power, 0.0)) >= 0.9 / 255.0)).any():
            rows.append(int(i))
    return tuple(rows), int(visible.size)


def cancel_closed_form():
    """Case "cancel" without autograd: one Gaussian, constant dL/dpixel, background 0.  With alpha_p = o exp(-q_p / 2) below the
    0.99 clamp, L = C sum_p alpha_p over the pixels with alpha_p >= 1/255, C = sum_c dL/dpixel_c colour_c, so the pixel's share
    of dL/d(mean, in pixels) is C alpha_p conic (x_p - mean), and the NDC scale is (0.5 W, 0.5 H).  Returns (abs (2,), signed (2,))."""
    from tests import aa_ref
    case = cases.make("cancel")
    cam, cloud = case["cam"], case["cloud"]
    tfx, tfy = cases.tan_fov(cam)
    H, W = cam.image_height, cam.image_width
    a0, b, c0, _ = aa_ref.cov2d64(cloud["means3D"], cam.world_view_transform, tfx, tfy, W, H, cloud["scales"], cloud["rotations"])
    a, b, c = float(a0[0]) + 0.3, float(b[0]), float(c0[0]) + 0.3
    det = a * c - b * b
    ka, kb, kc = c / det, -b / det, a / det
    hom = torch.cat([cloud["means3D"][0].double(), torch.ones(1, dtype=torch.float64)]) @ cam.full_proj_transform.double()
    w = 1.0 / (float(hom[3]) + 0.0000001)
    mx, my = ((float(hom[0]) * w + 1.0) * W - 1.0) * 0.5, ((float(hom[1]) * w + 1.0) * H - 1.0) * 0.5
    colour = np.maximum(0.28209479177387814 * cloud["shs"][0, 0].double().numpy() + 0.5, 0.0)       # degree-1 terms are zero
    C = float((case["g_color"][:, 0, 0].double().numpy() * colour).sum())
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dx, dy = mx - xs, my - ys
    power = -0.5 * (ka * dx * dx + kc * dy * dy) - kb * dx * dy
    alpha = float(cloud["opacities"][0, 0]) * np.exp(power)
    alpha = np.where((power <= 0) & (alpha >= 1.0 / 255.0), alpha, 0.0)
    gx = -C * alpha * (ka * dx + kb * dy) * (0.5 * W)
    gy = -C * alpha * (kc * dy + kb * dx) * (0.5 * H)
    return np.array([np.abs(gx).sum(), np.abs(gy).sum()]), np.array([gx.sum(), gy.sum()])
