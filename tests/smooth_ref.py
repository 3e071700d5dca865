"""References of the edge-aware smoothness term (test helper, not collected): include/lucid_raster.h, lr_smooth_args.

    reference(...)   the definition in float64 numpy: value, count and the analytic gradient (sign of each difference)
    restate32(...)   the header's operations in the header's number formats -- float32 guide mean, expf, gather sums and k,
                     double differences -- with the gather in the header's order ("header") or its reverse ("reverse"): the two
                     calibrators of the GPU test's bars, as normal_ref.closed_form is for the normals
    make_case(...)   the inputs of the kernel tests

Both evaluate the same vectorised walk over the terms (_evaluate), in float64 or in the header's formats."""
import numpy as np

GAMMA = 2.5
WEIGHT = 0.7
STEP = (0.6, 0.3, 0.45)             # heights of the guide's vertical step edge, per channel; the horizontal one is half as high


def _cut(a, axis, lo, hi):
    """a[..., lo:hi along `axis`, ...] of a [C,H,W] or [H,W] array; axis counts from the end (-1: x, -2: y)."""
    idx = [slice(None)] * a.ndim
    idx[axis] = slice(lo, hi)
    return a[tuple(idx)]


def _evaluate(map_, guide, mask, order, space, positive_only, gamma, weight, upstream, f, gather="header"):
    """f = np.float64: the definition; f = np.float32: the header's operations.  map_ [C,H,W], guide [G,H,W] or None, mask [H,W]
    or None.  Returns dict(value, count, grad [C,H,W], counted_x, counted_y)."""
    assert order in (1, 2) and space in ("depth", "inverse") and gather in ("header", "reverse")
    map_ = np.asarray(map_)
    C, H, W = map_.shape
    inverse = space == "inverse"
    assert not inverse or (C == 1 and positive_only)
    with np.errstate(all="ignore"):
        valid = np.isfinite(map_).all(axis=0)
        if positive_only:
            valid &= map_[0] > 0
        if mask is not None:
            valid &= np.asarray(mask) > 0
        # INVERSE space: u IS the quotient in the map's own format -- the header's one float32 division for the float32 maps of
        # the kernel tests (its rounding is part of the definition: the signs are those of the differences of THESE values), a
        # float64 division for the float64 maps of the finite-difference test
        u = ((map_.dtype.type(1) / map_) if inverse else map_).astype(f)
        if inverse:
            valid &= np.isfinite(u[0])
        u64 = u.astype(np.float64)                       # the differences are double in either form
        I = None if guide is None else np.asarray(guide).astype(f)
        k = (f(upstream) * f(weight)) / f(H * W)
        total, count = 0.0, 0
        steps, counted_maps = [], {}
        for axis in (-1, -2):                            # horizontal terms, then vertical ones
            n = u.shape[axis]
            if order == 1:
                parts = [(0, n - 1), (1, n)]            # p, q
                coefs = [-1.0, 1.0]
            else:
                parts = [(0, n - 2), (1, n - 1), (2, n)]          # m, p, q
                coefs = [1.0, -2.0, 1.0]
            if n < order + 1:
                counted_maps[axis] = np.zeros((0, 0), bool)
                continue
            us = [_cut(u64, axis, lo, hi) for lo, hi in parts]
            vs = [_cut(valid, axis, lo, hi) for lo, hi in parts]
            D = us[1] - us[0] if order == 1 else (us[0] - 2.0 * us[1]) + us[2]
            ok = np.logical_and.reduce(vs)
            if I is None:
                w = np.ones(ok.shape, f)
            else:
                Is = [_cut(I, axis, lo, hi) for lo, hi in parts]
                if order == 1:
                    a_g = np.abs(Is[0] - Is[1])
                else:
                    a_g = np.maximum(np.abs(Is[1] - Is[0]), np.abs(Is[2] - Is[1]))         # np.maximum keeps a NaN
                a = a_g[0] if I.shape[0] == 1 else ((a_g[0] + a_g[1]) + a_g[2]) / f(3)
                ok &= (a >= 0) & (a < np.inf)               # finite: a NaN and +inf both exclude the term
                w = np.exp(-(f(gamma) * a)).astype(f)
            w = np.where(ok, w, f(0))
            counted_maps[axis] = ok
            total += float((w.astype(np.float64) * np.where(ok, np.abs(D).sum(axis=0), 0.0)).sum())
            count += int(ok.sum())
            sign = np.where(ok[None], np.sign(D), 0.0).astype(f)
            # the gather's steps in the header's order: the term in which the pixel is q (m at order 2 comes last: the triple
            # centred on x + 1), i.e. terms from left to right / top to bottom as seen from the pixel
            for (lo, hi), coef in reversed(list(zip(parts, coefs))):
                steps.append((axis, lo, hi, (f(coef) * w)[None] * sign))
        g = np.zeros((C, H, W), f)
        for axis, lo, hi, contrib in (steps if gather == "header" else reversed(steps)):
            tgt = _cut(g, axis, lo, hi)
            tgt += contrib
        g = k * g                                        # once, on the sum: integer cancellation stays exact
        if inverse:
            uu = np.where(valid[None], u, f(0))
            g = -(g * uu) * uu
        if f is np.float32:
            value = float(np.float32(weight) * np.float32(total / (float(H) * float(W))))
        else:
            value = float(weight) * total / (float(H) * float(W))
    return dict(value=value, count=count, grad=g, counted_x=counted_maps[-1], counted_y=counted_maps[-2], valid=valid)


def reference(map_, guide=None, mask=None, order=1, space="depth", positive_only=False, gamma=GAMMA, weight=WEIGHT, upstream=1.0):
    """The definition in float64 (of a float32 or float64 map: see INVERSE space in _evaluate)."""
    map_ = np.asarray(map_)
    return _evaluate(map_ if map_.dtype == np.float32 else map_.astype(np.float64), guide, mask, order, space, positive_only, gamma, weight, upstream, np.float64)


def restate32(map_, guide=None, mask=None, order=1, space="depth", positive_only=False, gamma=GAMMA, weight=WEIGHT, upstream=1.0,
              gather="header"):
    """The header's operations in the header's formats; gather: "header" order or its "reverse"."""
    map_ = np.asarray(map_)
    assert map_.dtype == np.float32
    return _evaluate(map_, guide, mask, order, space, positive_only, gamma, weight, upstream, np.float32, gather)


def make_case(H, W, seed, kind="smooth"):
    """dict(depth [H,W], vectors [3,H,W], guide [3,H,W], texture [3,H,W], mask [H,W]), float32.  depth in [0.5, 10] (inside the
    range in which the double differences are exact); smooth: a tilted plane plus a low-frequency bump, rand: uniform noise.  Images of 64
    pixels and more get about 5 % holes (zeros, a few NaNs, one +inf) and a mask with a hole block, a NaN and a negative value;
    every image gets runs of exactly equal neighbours (sign(0) = 0).  The guide is piecewise constant: a step edge of heights
    STEP through the middle column and one of half those heights through the middle row, so a term either lies in a flat region
    (a = 0, w = 1 exactly) or crosses an edge.  That is on purpose: a pixel's gradient is a signed sum of its terms' float32
    weights, and under a TEXTURED guide neighbouring weights that differ in their last digits cancel, which leaves a pixel with
    no digits of its own whatever the kernel does -- the per-pixel judge of the GPU test needs a guide without that, and
    `texture` (the same edges plus noise) is the guide of the test that holds the gradient to the tensor's scale instead.
    vectors: a unit vector field with a few NaN pixels, the C = 3 input."""
    assert kind in ("smooth", "rand")
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    if kind == "smooth":
        depth = 2.0 + 3.0 * xs + 2.0 * ys + 1.5 * np.exp(-((xs - 0.5) ** 2 + (ys - 0.45) ** 2) / 0.08)
        vec = np.stack([0.6 * np.sin(3.0 * xs + 1.0), 0.6 * np.cos(2.0 * ys), -1.0 - 0.2 * xs * ys])
    else:
        depth = rng.uniform(0.5, 10.0, (H, W))
        vec = rng.standard_normal((3, H, W))
    vec = vec / np.sqrt((vec * vec).sum(axis=0))
    depth = depth.astype(np.float32)
    vec = vec.astype(np.float32)
    guide = np.full((3, H, W), 0.2)
    guide[:, :, W // 2:] += np.array(STEP)[:, None, None]
    guide[:, H // 2:, :] += 0.5 * np.array(STEP)[:, None, None]
    texture = guide + rng.uniform(0.0, 0.15, (3, H, W))
    mask = np.ones((H, W), np.float32)
    # exactly equal neighbours: runs of three, horizontal and vertical (as long as the image has room)
    for _ in range(max(1, H * W // 200)):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        depth[y, x:x + 3] = depth[y, x]
        vec[:, y, x:x + 3] = vec[:, y, x][:, None]
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        depth[y:y + 3, x] = depth[y, x]
        vec[:, y:y + 3, x] = vec[:, y, x][:, None]
    if H * W >= 64:
        holes = rng.random((H, W)) < 0.05
        depth[holes] = 0.0
        pick = lambda: (int(rng.integers(0, H)), int(rng.integers(0, W)))
        for _ in range(3):
            depth[pick()] = np.nan
            vec[(slice(None),) + pick()] = np.nan
        depth[pick()] = np.inf
        by, bx = H // 4, W // 3
        mask[by:by + max(1, H // 5), bx:bx + max(1, W // 6)] = 0.0
        mask[pick()] = np.nan
        mask[pick()] = -1.0
    return dict(depth=depth, vectors=vec, guide=guide.astype(np.float32), texture=texture.astype(np.float32), mask=mask)
