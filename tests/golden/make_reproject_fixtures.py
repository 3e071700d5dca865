"""Writes tests/golden/ref_reproject_fixtures.npz: what the reference's own host code makes of small clouds.

Run in the build container only (it needs scipy); the tests read the .npz and never scipy.  reference_frame() below follows
R/luciddreamer.py line by line, with the reference's own scipy calls and arguments:
    :386-387  camera and pixel coordinates of the whole cloud, float64, R.dot(X) + T through BLAS
    :389-395  valid_idx (closed bounds), the projected coordinates and their np.round as int32
    :399      scipy.interpolate.griddata(method='linear', fill_value=0) onto the pixel grid
              (stored BEFORE the edgemask patch of :400, which has no counterpart in the library)
    :402-405  the hit plane and scipy.ndimage.maximum_filter(size=(9,9), axes=(0,1))
    :406-408  unhit pixels marked -1, scipy.ndimage.minimum_filter(size=(11,11), axes=(0,1)) of (sum != -3)
    :411-414  mask_hf, border_valid_idx
Cases: two random clouds in two depth layers (48x64 and 37x53), the second also with one constant colour, and a lifted grid
(:370-371) seen from its own pose, where every projected coordinate is integral.

    python tests/golden/make_reproject_fixtures.py
"""
import os

import numpy as np
from scipy.interpolate import griddata as interp_grid
from scipy.ndimage import maximum_filter, minimum_filter

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_frame(X, C, K, R, T, H, W, check_margins=True):
    """The reference's host pipeline for one pose, in its operations and with its scipy arguments (the line numbers above)."""
    cam = R.dot(X) + T                                           # :386, float64 through BLAS
    q = np.matmul(K, cam)                                        # :387
    with np.errstate(all="ignore"):
        u, v = q[0] / q[2], q[1] / q[2]
    if check_margins:
        # the library forms R X + T elementwise, the reference through BLAS: no point of a fixture may sit where a last-bit
        # difference could change a comparison or a rounding
        assert np.abs(q[2]).min() > 1e-12
        for c, hi in ((u, W - 1), (v, H - 1)):
            to_half = np.abs((c - 0.5) - np.round(c - 0.5))
            assert to_half.min() > 1e-9 and np.abs(c).min() > 1e-9 and np.abs(c - hi).min() > 1e-9
    valid_idx = np.where((q[2] > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1))[0]      # :389-393
    uv = np.stack([u[valid_idx], v[valid_idx]])                  # :394
    rounded = np.round(uv).astype(np.int32)                      # :395

    gx, gy = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    targets = np.stack((gx, gy), axis=-1).reshape(-1, 2)
    image = interp_grid(uv.T, C[valid_idx], targets, method="linear", fill_value=0).reshape(H, W, 3)      # :399

    hit = np.zeros((H, W), dtype=np.float32)
    hit[rounded[1], rounded[0]] = 1                              # :402-403
    dil = maximum_filter(hit, size=(9, 9), axes=(0, 1))          # :405
    marked = dil[..., None] * image + (1 - dil[..., None]) * (-1)                                       # :406
    mask = minimum_filter((marked.sum(-1) != -3) * 1, size=(11, 11), axes=(0, 1))                       # :408

    down = np.abs(mask[:H - 1, :W - 1] - mask[1:, :W - 1])       # :411-413
    right = np.abs(mask[:H - 1, :W - 1] - mask[:H - 1, 1:])
    hf = np.where(np.pad(down + right, ((0, 1), (0, 1)), "edge") < 0.3, 0, 1)
    border_valid_idx = np.where(hf[rounded[1], rounded[0]] == 1)[0]                                     # :414
    return dict(valid_idx=valid_idx.astype(np.int64), round_coord=rounded, hit=hit.astype(np.uint8),
                round_mask=dil.astype(np.uint8), mask2=mask.astype(np.uint8), mask_hf=hf.astype(np.uint8),
                border_valid_idx=border_valid_idx.astype(np.int64), griddata=image)


def pose(rng):
    a, b, c = rng.uniform(-0.08, 0.08, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rx @ Ry @ Rz, rng.uniform(-0.1, 0.1, (3, 1))


def random_cloud(rng, N, H, W):
    """Two depth layers that cover about two thirds of the view, a sparse sprinkle over the rest, and points that fall off
    screen or behind the camera."""
    K = np.array([[0.9 * W, 0, W / 2.0], [0, 0.9 * W, H / 2.0], [0, 0, 1]], dtype=np.float64)
    R, T = pose(rng)
    n_sparse = 25
    u = np.concatenate([rng.uniform(-6, 0.68 * W, N - n_sparse), rng.uniform(0.7 * W, W + 4, n_sparse)])
    v = rng.uniform(-6, H + 5, N)
    z = np.where(rng.random(N) < 0.5, rng.uniform(2.8, 3.2, N), rng.uniform(5.5, 6.5, N))
    z[rng.random(N) < 0.02] *= -1                                        # behind the camera
    cam = np.linalg.inv(K) @ np.stack([u * z, v * z, z])
    X = (np.linalg.inv(R) @ (cam - T)).astype(np.float32)                # [3, N], as pts_coord_world
    C = rng.random((N, 3)).astype(np.float32)
    return X, C, K, R, T


def lifted_grid(rng, H, W):
    """The lift of :370-371 for a depth map of powers of two and a power-of-two focal length at the identity pose: the lifted
    float32 points are exact, so their projection at the same pose lands on the pixel centres exactly."""
    K = np.array([[32, 0, W / 2], [0, 32, H / 2], [0, 0, 1]], dtype=np.float64)
    depth = np.where(rng.random((H // 8, W // 8)) < 0.5, 2.0, 4.0).astype(np.float32).repeat(8, 0).repeat(8, 1)
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    rays = np.stack((gx * depth, gy * depth, depth), axis=0).reshape(3, -1)
    X = np.matmul(np.linalg.inv(K), rays).astype(np.float32)             # inv(R0) = I, T0 = 0
    C = rng.integers(0, 256, (H * W, 3)).astype(np.float32) / 255.
    return X, C, K, np.eye(3), np.zeros((3, 1)), depth


def main():
    rng = np.random.default_rng(20240611)
    out = {}
    for name, (H, W, N) in {"a": (48, 64, 3000), "b": (37, 53, 2003)}.items():
        X, C, K, R, T = random_cloud(rng, N, H, W)
        ref = reference_frame(X, C, K, R, T, H, W)
        assert 0 < ref["mask2"].sum() < H * W and ref["border_valid_idx"].size > 0 and ref["valid_idx"].size < N
        out.update({f"{name}_{k}": v for k, v in dict(X=X, C=C, K=K, R=R, T=T, HW=np.array([H, W])).items()})
        out.update({f"{name}_{k}": (v.astype(np.float32) if k == "griddata" else v) for k, v in ref.items()})
        if name == "b":
            const = np.array([0.25, 0.5, 0.8125], dtype=np.float32)
            out["b_const_color"] = const
            out["b_const_griddata"] = reference_frame(X, np.tile(const, (N, 1)), K, R, T, H, W)["griddata"]
    H, W = 48, 64
    X, C, K, R, T, depth = lifted_grid(rng, H, W)
    ref = reference_frame(X, C, K, R, T, H, W, check_margins=False)       # integral on purpose: exact in both evaluation orders
    assert np.array_equal(ref["round_coord"][0] + W * ref["round_coord"][1], np.arange(H * W)) and ref["mask2"].all()
    out.update({f"grid_{k}": v for k, v in dict(X=X, C=C, K=K, R=R, T=T, HW=np.array([H, W]), depth=depth).items()})
    out.update({f"grid_{k}": v for k, v in ref.items()})
    path = os.path.join(HERE, "ref_reproject_fixtures.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
