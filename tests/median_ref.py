"""Reference of the median depth / id outputs (lr_render_median), in numpy, on the CPU oracle's own state.

The per-pixel walk of the blend forward, taken from the oracle's stage() -- ranges, point_list, means2D, conic_opacity, depths --
in float32 operations in the reference's order (oracle/raster_oracle.c, forward.cu:331-347), T = 1 at the start:
    power > 0 -> skip;  alpha = min(0.99, opacity exp(power)), alpha < 1/255 -> skip;
    test_T = T (1 - alpha), test_T < 1e-4 -> stop, not blended;  otherwise blend, T = test_T.
The median Gaussian of a pixel is the first blended Gaussian with test_T < 0.5.

A pixel is FRAGILE -- two correct float32 evaluations may pick different Gaussians -- if, before its median is found,
  * some blended test_T lies within T_BAND = 4e-5 of 0.5 (4 x helpers.COLOR_ATOL, the project's own bound on what T may be off by),
  * some alpha with power <= 0 lies within a relative ALPHA_BAND = 1e-4 of 1/255, or
  * the oracle's own fragile bits are set.
"""
import functools

import numpy as np
import torch

from tests import helpers as hp

T_BAND = 4 * hp.COLOR_ATOL
ALPHA_BAND = 1e-4
# P, W, H, scale_mult of helpers.box_setup(seed=0): the three inputs of the median tests
INPUTS = {"sparse": (2000, 70, 45, 1.0), "dense": (3000, 48, 40, 6.0), "small": (400, 33, 20, 3.0)}
PARITY_INPUTS = ("sparse", "dense")       # fragile share <= FRAGILE_CAP (tests/test_median_cpu.py); "small" is over it
FRAGILE_CAP = 0.005
BG = (0.0, 0.1, 0.2)
DEGREE = 3


def walk(st, W, H):
    """(ids [H,W] int32 (-1: none), depth [H,W] float32 (0: none), fragile [H,W] bool) from an oracle result's stage()."""
    f32 = np.float32
    gx = (W + 15) // 16
    gy = (H + 15) // 16
    ids = np.full((H, W), -1, np.int32)
    fragile = st["fragile"] != 0
    m2, co, plist = st["means2D"], st["conic_opacity"], st["point_list"]
    thr = f32(1.0) / f32(255.0)
    for tile in range(gx * gy):
        tx, ty = tile % gx, tile // gx
        ys, xs = np.mgrid[ty * 16:min(H, ty * 16 + 16), tx * 16:min(W, tx * 16 + 16)]
        ys, xs = ys.ravel(), xs.ravel()
        pxf, pyf = xs.astype(f32), ys.astype(f32)
        T = np.ones(xs.size, f32)
        active = np.ones(xs.size, bool)
        med = np.full(xs.size, -1, np.int32)
        frag = np.zeros(xs.size, bool)
        r0, r1 = (int(v) for v in st["ranges"][tile])
        for k in range(r0, r1):
            if not active.any():
                break
            g = int(plist[k])
            dx, dy = m2[g, 0] - pxf, m2[g, 1] - pyf
            a, b, c, op = (f32(v) for v in co[g])
            power = f32(-0.5) * (a * dx * dx + c * dy * dy) - b * dx * dy
            ok = power <= 0
            with np.errstate(over="ignore"):
                alpha = np.minimum(f32(0.99), op * np.exp(power))
            frag |= active & ok & (np.abs(alpha.astype(np.float64) - 1.0 / 255.0) <= ALPHA_BAND / 255.0)
            use = active & ok & (alpha >= thr)
            test_T = T * (f32(1.0) - alpha)
            stop = use & (test_T < f32(0.0001))
            blend = use & ~stop
            frag |= blend & (np.abs(test_T.astype(np.float64) - 0.5) <= T_BAND)
            found = blend & (test_T < f32(0.5))
            med[found] = g
            T = np.where(blend, test_T, T)
            active &= ~(stop | found)
        ids[ys, xs] = med
        fragile[ys, xs] |= frag
    depth = np.where(ids >= 0, st["depths"][np.maximum(ids, 0)], f32(0)).astype(f32)
    return ids, depth, fragile


def grad_means3D(ids, G, viewmatrix, P):
    """float64 dL/dmeans3D [P,3] of sum(median_depth * G) for the given ids: d median_depth[p] / d z_g = 1 for g = ids[p], through
    z = view[2] x + view[6] y + view[10] z + view[14] (flat, column-major view matrix).  Also the pixel count and sum |G| per row."""
    ids = np.asarray(ids).reshape(-1)
    G = np.asarray(G, np.float64).reshape(-1)
    v = np.asarray(viewmatrix, np.float64).reshape(-1)[[2, 6, 10]]
    has = ids >= 0
    s = np.bincount(ids[has], weights=G[has], minlength=P)
    n = np.bincount(ids[has], minlength=P)
    sabs = np.bincount(ids[has], weights=np.abs(G[has]), minlength=P)
    return s[:, None] * v[None, :], n, sabs


@functools.lru_cache(maxsize=None)
def box_input(name):
    P, W, H, s = INPUTS[name]
    return hp.box_setup(P, W, H, seed=0, scale_mult=s)


@functools.lru_cache(maxsize=None)
def box_reference(name):
    """The oracle's forward of an input and the walk on it, computed once and shared: dict(ref, st, ids, depth, fragile)."""
    cam, cloud = box_input(name)
    ref = hp.run_oracle(cloud, cam, DEGREE, torch.tensor(BG))
    st = ref["res"].stage()
    ids, depth, fragile = walk(st, cam.image_width, cam.image_height)
    for a in (ids, depth, fragile):
        a.setflags(write=False)
    return dict(ref=ref, st=st, ids=ids, depth=depth, fragile=fragile)
