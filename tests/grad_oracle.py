"""Float64 PyTorch restatement of oracle/torch_oracle.render with DIFFERENTIABLE depth and alpha outputs (test helper, not
collected).

The depth-mode backward (lr_view_backward with dL_depths and depth_image, config.set_depth_gradient) returns the true derivative of the forward's depth
output depth = D / acc (0 where acc <= 0.5) with the colour path's conventions -- the 0.99 clamp of alpha and the fov clamp
treated as in torch_oracle (its docstring, points i and ii), the skips, the T < 1e-4 stop, the sort order and the acc > 0.5
mask constant.  torch_oracle reproduces the reference, whose depth carries no gradient (point iii: two detach() calls, on the
per-Gaussian view depth and on the depth image); this restatement of its render loop drops exactly those two, so that
autograd through it is the contract of the depth mode.  The sort key stays detached.

The alpha output (return_alpha, lr_render_alpha) is 1 - T_final per pixel; its backward (lr_view_backward with dL_dalpha) is the true
derivative of 1 - prod_i (1 - alpha_i) over the layers the forward applied, with the same conventions (the T < 1e-4 stop's
trigger is not applied).
"""
import torch

from oracle.torch_oracle import cov3d_from_scale_rot, sh_to_rgb


def render(means3D, opacities, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, bg,
           scales=None, rotations=None, scale_modifier=1.0, cov3D_precomp=None,
           shs=None, degree=0, colors_precomp=None, means2D=None, dtype=torch.float64, detach_depth=False, alpha=False,
           with_layers=False, pixel_probe=None):
    """oracle.torch_oracle.render with a differentiable depth output: returns (color (3,H,W), depth (1,H,W), radii (P,)
    int32).  detach_depth=True puts back the two detach() calls of torch_oracle (its docstring, point iii).
    alpha=True: (color, depth, alpha (1,H,W), radii), alpha = 1 - T_final differentiable.
    with_layers=True appends a list of per-tile dicts {ids, contrib, alpha, T_fin, pix} (the applied layers of every pixel of
    the tile, detached) for closed-form checks.
    pixel_probe: a list; every non-empty tile appends (ids, (ys, xs), E) with E a zero leaf [256, len(ids), 2] added to every
    pixel's own offset (dx, dy) to the Gaussians of the tile, so that dL/dE[p, k] is the share of dL/d(mean of ids[k], in pixels)
    that flows through pixel p -- all shares from one backward."""
    cv = lambda t: None if t is None else t.to(dtype)
    means3D, opacities, scales, rotations = cv(means3D), cv(opacities), cv(scales), cv(rotations)
    cov3D_precomp, shs, colors_precomp, means2D = cv(cov3D_precomp), cv(shs), cv(colors_precomp), cv(means2D)
    V, Pm, campos, bg = cv(viewmatrix), cv(projmatrix), cv(campos), cv(bg)
    P = means3D.shape[0]
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    gx, gy = (W + 15) // 16, (H + 15) // 16

    p_view = means3D @ V[:3, :3] + V[3, :3]                       # auxiliary.h:58-66
    hom = means3D @ Pm[:3, :] + Pm[3, :]                           # auxiliary.h:68-77
    p_w = 1.0 / (hom[:, 3] + 0.0000001)
    ndc = hom[:, :3] * p_w[:, None]
    if means2D is not None:                                        # virtual screen-space offsets (NDC units)
        ndc = torch.cat([ndc[:, :2] + means2D[:, :2], ndc[:, 2:3]], dim=1)
    in_front = p_view[:, 2] > 0.2                                  # auxiliary.h:154

    cov3D = cov3D_precomp if cov3D_precomp is not None else cov3d_from_scale_rot(scales, scale_modifier, rotations)

    # forward.cu:74-113 with the backward's clamp convention (module docstring (ii))
    tz = p_view[:, 2]
    tz_safe = torch.where(in_front, tz, torch.ones_like(tz))
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = p_view[:, 0] / tz_safe, p_view[:, 1] / tz_safe
    tx = torch.where((txtz < -limx) | (txtz > limx), (txtz.clamp(-limx, limx) * tz_safe).detach(), p_view[:, 0])
    ty = torch.where((tytz < -limy) | (tytz > limy), (tytz.clamp(-limy, limy) * tz_safe).detach(), p_view[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz_safe, zero, -(fx * tx) / (tz_safe * tz_safe),
                     zero, fy / tz_safe, -(fy * ty) / (tz_safe * tz_safe)], dim=1).reshape(P, 2, 3)
    Wc = V[:3, :3].T                                               # world->camera rotation
    A = J @ Wc
    Sig = torch.stack([cov3D[:, 0], cov3D[:, 1], cov3D[:, 2], cov3D[:, 1], cov3D[:, 3], cov3D[:, 4],
                       cov3D[:, 2], cov3D[:, 4], cov3D[:, 5]], dim=1).reshape(P, 3, 3)
    cov2 = A @ Sig @ A.transpose(1, 2)
    a, b, c = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    ok = in_front & (det != 0)
    det_s = torch.where(ok, det, torch.ones_like(det))
    conic = torch.stack([c / det_s, -b / det_s, a / det_s], dim=1)
    mid = 0.5 * (a + c)
    lam = mid + torch.sqrt(torch.clamp_min(mid * mid - det, 0.1))
    radius = torch.ceil(3.0 * torch.sqrt(lam)).detach()
    px = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5                       # auxiliary.h:41-44
    py = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    ri = radius.to(torch.int64).to(dtype)
    trunc = lambda t: torch.trunc(t.detach()).to(torch.int64)      # C (int) cast
    rminx = trunc((px - ri) / 16).clamp(0, gx); rmaxx = trunc((px + ri + 15) / 16).clamp(0, gx)
    rminy = trunc((py - ri) / 16).clamp(0, gy); rmaxy = trunc((py + ri + 15) / 16).clamp(0, gy)
    ok = ok & (((rmaxx - rminx) * (rmaxy - rminy)) > 0)
    radii = torch.where(ok, radius, torch.zeros_like(radius)).to(torch.int32)

    if colors_precomp is not None:
        rgb = colors_precomp
    else:
        d = means3D - campos[None, :]
        rgb = sh_to_rgb(degree, shs, d / d.norm(dim=1, keepdim=True))
    depth_g = p_view[:, 2].detach() if detach_depth else p_view[:, 2]     # view depth z (torch_oracle: detached)
    op = opacities.reshape(-1)

    # stable order by (float32 depth bits, index): rasterizer_impl.cu:98-108, 304-309
    order_all = torch.argsort(depth_g.detach().to(torch.float32), stable=True)       # the sort key stays a constant
    out_c = [[None] * gx for _ in range(gy)]
    out_d = [[None] * gx for _ in range(gy)]
    out_a = [[None] * gx for _ in range(gy)]
    layers = []
    for ty_ in range(gy):
        for tx_ in range(gx):
            sel = ok & (rminx <= tx_) & (tx_ < rmaxx) & (rminy <= ty_) & (ty_ < rmaxy)
            ids = order_all[sel[order_all]]
            ys, xs = torch.meshgrid(torch.arange(ty_ * 16, ty_ * 16 + 16), torch.arange(tx_ * 16, tx_ * 16 + 16),
                                    indexing="ij")
            pxf, pyf = xs.reshape(-1).to(dtype), ys.reshape(-1).to(dtype)
            if ids.numel() == 0:
                c_t = bg[:, None].expand(3, 256)
                d_t = torch.zeros(256, dtype=dtype)
                a_t = torch.zeros(256, dtype=dtype)
            else:
                dx = px[ids][None, :] - pxf[:, None]
                dy = py[ids][None, :] - pyf[:, None]
                if pixel_probe is not None:
                    E = torch.zeros(256, ids.numel(), 2, dtype=dtype, requires_grad=True)
                    dx, dy = dx + E[:, :, 0], dy + E[:, :, 1]
                    pixel_probe.append((ids, (ys.reshape(-1), xs.reshape(-1)), E))
                cn = conic[ids]
                power = -0.5 * (cn[:, 0][None] * dx * dx + cn[:, 2][None] * dy * dy) - cn[:, 1][None] * dx * dy
                G = torch.exp(torch.clamp_max(power, 0.0))
                araw = op[ids][None, :] * G
                alpha_i = araw + (torch.clamp_max(araw, 0.99) - araw).detach()     # torch_oracle docstring (i)
                valid = (power <= 0) & (alpha_i.detach() >= 1.0 / 255.0)
                a_eff = torch.where(valid, alpha_i, torch.zeros_like(alpha_i))
                one_m = 1.0 - a_eff
                T_incl = torch.cumprod(one_m, dim=1)
                T_excl = torch.cat([torch.ones_like(T_incl[:, :1]), T_incl[:, :-1]], dim=1)
                stop = valid & (T_incl.detach() < 0.0001)
                done = torch.cumsum(stop.to(torch.int64), dim=1) > 0                # inclusive: stopper not applied
                contrib = valid & ~done
                w = torch.where(contrib, alpha_i * T_excl, torch.zeros_like(alpha_i))
                # T after the last applied Gaussian
                T_fin = torch.prod(torch.where(contrib, one_m, torch.ones_like(one_m)), dim=1)
                c_t = (w @ rgb[ids]).T + T_fin[None, :] * bg[:, None]
                acc = 0.000001 + w.sum(dim=1)
                Dacc = w @ depth_g[ids]
                d_t = torch.where(acc > 0.5, Dacc / acc, torch.zeros_like(acc))    # the mask acc > 0.5 is a constant
                if detach_depth:
                    d_t = d_t.detach()
                a_t = 1.0 - T_fin                                                   # the alpha output
                if with_layers:
                    layers.append(dict(ids=ids, contrib=contrib, alpha=alpha_i.detach(), T_fin=T_fin.detach(),
                                       pix=(ys.reshape(-1), xs.reshape(-1))))
            out_c[ty_][tx_] = c_t.reshape(3, 16, 16)
            out_d[ty_][tx_] = d_t.reshape(1, 16, 16)
            out_a[ty_][tx_] = a_t.reshape(1, 16, 16)
    cat = lambda out: torch.cat([torch.cat(row, dim=2) for row in out], dim=1)[:, :H, :W]
    res = (cat(out_c), cat(out_d)) + ((cat(out_a),) if alpha else ()) + (radii,)
    return res + (layers,) if with_layers else res
