"""Plain numpy restatement of luciddreamer_amd.reproject (csrc/reproject.hip), operation for operation.

Every float64 expression is written elementwise in the order the header documents (include/lucid_raster.h, lr_reproject), so
numpy forms the same bits as the device: no BLAS, no fused multiply-add.  The order-dependent parts are integer sums
(np.add.at on uint64, np.minimum.at on the uint32 bits of z), which do not depend on the order.

    project(X, C, K, R, T, H, W, z_tolerance) -> dict(valid, pix, hit, dil, mask, border, zmin, A, S, image, image_u8, depth)
    lift(depth, K, R, T)                      -> float32 [3, H*W]
    compose_pose(Ri2j, Ti2j, Rw2i, Tw2i), pc2w(Rw2j, Tw2j): the pose algebra of R/luciddreamer.py:527-534
"""
import numpy as np

NO_HIT = np.uint32(0xFFFFFFFF)


def _xyz(X):
    X = np.asarray(X, dtype=np.float32)
    if X.ndim != 2 or 3 not in X.shape:
        raise ValueError(X.shape)
    if X.shape[1] != 3:                          # [3, N]; a 3 x 3 array is read as [N, 3]
        X = X.T
    return X[:, 0].astype(np.float64), X[:, 1].astype(np.float64), X[:, 2].astype(np.float64)


def _rows(M, a, b, c):
    """((M_i0 a + M_i1 b) + M_i2 c) for the three rows of M."""
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    return [(M[i, 0] * a + M[i, 1] * b) + M[i, 2] * c for i in range(3)]


def project_points(X, K, R, T, H, W):
    """(valid, iu, iv, u, v, z32, q2): the per-point part."""
    x, y, z = _xyz(X)
    T = np.asarray(T, dtype=np.float64).reshape(3)
    with np.errstate(all="ignore"):
        p = [r + T[i] for i, r in enumerate(_rows(R, x, y, z))]
        q = _rows(K, p[0], p[1], p[2])
        u, v = q[0] / q[2], q[1] / q[2]
        valid = (q[2] > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        iu = np.where(valid, np.rint(u), 0).astype(np.int64)
        iv = np.where(valid, np.rint(v), 0).astype(np.int64)
        z32 = q[2].astype(np.float32)
    return valid, iu, iv, u, v, z32, q[2]


def window(plane, radius, op):
    """op (np.maximum / np.minimum) over the (2 radius + 1)^2 window clamped to the image."""
    H, W = plane.shape
    out = plane.copy()
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, ye = max(0, -dy), min(H, H - dy)
            xs, xe = max(0, -dx), min(W, W - dx)
            if ys < ye and xs < xe:
                out[ys:ye, xs:xe] = op(out[ys:ye, xs:xe], plane[ys + dy:ye + dy, xs + dx:xe + dx])
    return out


def window_sum(plane, radius):
    """Integer sums over the clamped window (uint64)."""
    H, W = plane.shape[:2]
    out = np.zeros_like(plane)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, ye = max(0, -dy), min(H, H - dy)
            xs, xe = max(0, -dx), min(W, W - dx)
            if ys < ye and xs < xe:
                out[ys:ye, xs:xe] += plane[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def border_of(mask):
    """The reference's mask_hf (R/luciddreamer.py:411-413) as 0 / 1."""
    m = mask.astype(np.int64)
    H, W = m.shape
    hf = np.abs(m[:H - 1, :W - 1] - m[1:, :W - 1]) + np.abs(m[:H - 1, :W - 1] - m[:H - 1, 1:])
    hf = np.pad(hf, ((0, 1), (0, 1)), "edge")
    return np.where(hf < 0.3, 0, 1).astype(np.uint8)


def project(X, C, K, R, T, H, W, z_tolerance=0.05):
    valid, iu, iv, u, v, z32, _ = project_points(X, K, R, T, H, W)
    N = valid.shape[0]
    HW = H * W
    pix = np.where(valid, iv * W + iu, -1).astype(np.int32)
    vi = np.nonzero(valid)[0]

    zbits = np.full(HW, NO_HIT, dtype=np.uint32)
    np.minimum.at(zbits, pix[vi], z32[vi].view(np.uint32))
    hit = (zbits != NO_HIT).astype(np.uint8).reshape(H, W)
    zmin = np.where(zbits == NO_HIT, np.uint32(0x7F800000), zbits).view(np.float32)
    dil = window(hit, 4, np.maximum)
    mask = window(dil, 5, np.minimum)
    border = border_of(mask)

    # the z-tested bilinear splat in fixed point
    C = np.asarray(C, dtype=np.float32).reshape(N, 3)
    c = np.where(C > 0, C, np.float32(0))                      # NaN -> 0
    c = np.where(c < 1, c, np.float32(1))
    cq = np.rint(c.astype(np.float64) * 65535.0).astype(np.uint64)
    zt = np.float32(1) + np.float32(z_tolerance)               # float32 sum
    A = np.zeros((HW, 4), dtype=np.uint64)                     # A_r, A_g, A_b, S
    uu, vv, zz = u[vi], v[vi], z32[vi]
    x0, y0 = np.floor(uu), np.floor(vv)
    fx, fy = uu - x0, vv - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            w = (fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy)
            wq = np.rint(w * 65536.0).astype(np.uint64)
            xx, yy = x0 + dx, y0 + dy
            inside = (xx <= W - 1) & (yy <= H - 1)
            p = np.where(inside, yy * W + xx, 0)
            with np.errstate(all="ignore"):
                ok = inside & (zz <= zmin[p] * zt)             # float32 multiply
            contrib = np.concatenate([wq[:, None] * cq[vi], wq[:, None]], axis=1)
            np.add.at(A, p[ok], contrib[ok])
    A = A.reshape(H, W, 4)
    fill = window_sum(A, 4)
    use = np.where((A[..., 3:4] == 0), fill, A)
    S = use[..., 3].astype(np.float64)
    with np.errstate(all="ignore"):
        img = ((use[..., :3].astype(np.float64) / S[..., None]) / 65535.0).astype(np.float32)
    image = np.where(mask[..., None] == 1, img, np.float32(0)).astype(np.float32)
    image_u8 = np.rint(image * np.float32(255)).astype(np.uint8)
    zplane = zmin.reshape(H, W)
    depth = np.where((mask == 1) & np.isfinite(zplane), zplane, np.float32(0)).astype(np.float32)
    return dict(valid=valid.astype(np.uint8), pix=pix, hit=hit, dil=dil, mask=mask, border=border, zmin=zplane,
                A=A[..., :3], S=A[..., 3], image=image, image_u8=image_u8, depth=depth)


def lift_f64(depth, K, R, T):
    """float64 [3, H*W]: inv(R) (inv(K) (x d, y d, d)) - inv(R) T, elementwise in the documented order."""
    depth = np.asarray(depth, dtype=np.float32)
    H, W = depth.shape
    Ki = np.linalg.inv(np.asarray(K, dtype=np.float64).reshape(3, 3))
    Ri = np.linalg.inv(np.asarray(R, dtype=np.float64).reshape(3, 3))
    T = np.asarray(T, dtype=np.float64).reshape(3)
    t = [(Ri[i, 0] * T[0] + Ri[i, 1] * T[1]) + Ri[i, 2] * T[2] for i in range(3)]
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    d = depth.astype(np.float64).reshape(-1)
    xd, yd = x.reshape(-1) * d, y.reshape(-1) * d
    c = _rows(Ki, xd, yd, d)
    w = _rows(Ri, c[0], c[1], c[2])
    return np.stack([w[i] - t[i] for i in range(3)], axis=0)


def lift(depth, K, R, T):
    return lift_f64(depth, K, R, T).astype(np.float32)


def compose_pose(Ri2j, Ti2j, Rw2i, Tw2i):
    """R/luciddreamer.py:527-528."""
    Rw2j = np.matmul(Ri2j, Rw2i)
    Tw2j = np.matmul(Ri2j, Tw2i) + Ti2j
    return Rw2j, Tw2j


def pc2w(Rw2j, Tw2j):
    """R/luciddreamer.py:531-534."""
    yz_reverse = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]])
    Rj2w = np.matmul(yz_reverse, Rw2j).T
    Tj2w = -np.matmul(Rj2w, np.matmul(yz_reverse, Tw2j))
    P = np.concatenate((Rj2w, Tj2w), axis=1)
    return np.concatenate((P, np.array([[0, 0, 0, 1]])), axis=0)
