"""Writes tests/golden/ref_dream_fixtures.npz: what the reference's own host code makes of the steps between its networks and the
append of the new points, for two small clouds.

Run in the build container only (it needs scipy and torch); the tests read the .npz and never scipy.  reference_dream() below
follows R/luciddreamer.py with the reference's own operations, dtypes and scipy arguments:
    :386-414  the frame of the cloud at the new pose (make_reproject_fixtures.reference_frame)
    :430      trans3d: a float32 4x4 built from the VALUE of the scale, which therefore never receives a gradient: after the 100
              Adam steps of :429-440 it is the identity (asserted below on the first case, with the reference's own loop)
    :443-447  the border correspondences' depth lifted: inv(K) through torch.matmul, inv(R) as float32 (.float())
    :452-468  camera origin (float32), the foot of each cloud point on its camera ray, the depth offset
    :469-474  compensate_depth and pixel_cam2 with the four zero corners appended
    :477-479  scipy.interpolate.griddata, linear with the nearest fallback, at the hole pixels
    :481-490  the compensated lift and the colours of the appended points
The reference's K must be float32 for :443 to run at all (torch.matmul refuses mixed dtypes): the fixtures' K holds values that
float32 represents exactly.

    python tests/golden/make_dream_fixtures.py
"""
import os
import sys

import numpy as np
import torch
from scipy.interpolate import griddata as interp_grid

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reproject_fixtures import pose, reference_frame  # noqa: E402


def _rays(K, depth, W, H):
    """inv(K) as a tensor and the float32 stack (x d, y d, d) over the pixel grid, [3,H,W]: the operands of :431 / :443."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    d = torch.tensor(depth)
    return torch.tensor(np.linalg.inv(K)), torch.stack((torch.tensor(x) * d, torch.tensor(y) * d, 1 * d), axis=0)


def _world32(R, T, cam):
    """:432 / :444: inv(R) cast to float32 applied to the camera points, minus inv(R) float32 times T float32."""
    Rinv32 = torch.tensor(np.linalg.inv(R)).float()
    return Rinv32.matmul(cam) - Rinv32.matmul(torch.tensor(T).float())


def _apply(trans3d, world):
    """:433-435 / :445-447: homogeneous coordinates through the 4x4 and back."""
    h = torch.matmul(trans3d, torch.cat((world, torch.ones((1, world.shape[1]))), dim=0))
    return h[:3] / h[-1]


def adam_scale(K, R, T, H, W, depth_curr, round_coord, valid_idx, world, steps=100):
    """:424-440 in its operations: the scale after the loop, and whether it ever had a gradient.  The 4x4 is built, as there,
    by torch.tensor() from a nested list that holds the scale: a copy of its VALUE, a new leaf."""
    sc = torch.ones(1).float().requires_grad_(True)
    opt = torch.optim.Adam(params=[sc], lr=0.001)
    Kinv, rays = _rays(K, depth_curr, W, H)
    target = torch.tensor(world[:, valid_idx]).float()
    for _ in range(steps):
        rows = [[sc if r == c else 0 for c in range(4)] for r in range(3)] + [[0, 0, 0, 1]]
        trans3d = torch.tensor(rows).requires_grad_(True)
        cam = torch.matmul(Kinv, rays[:, round_coord[1], round_coord[0]].reshape(3, -1))
        loss = torch.mean((target - _apply(trans3d, _world32(R, T, cam))) ** 2)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return float(sc), sc.grad is not None


def reference_dream(X, K, R, T, H, W, depth_curr, image_curr, fr):
    """:443-493 for one pose; X is pts_coord_world [3,N] float32, K float32, R and T float64, depth_curr float32 [H,W]."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    valid_idx, round_coord, border_valid_idx, mask2 = fr["valid_idx"], fr["round_coord"], fr["border_valid_idx"], fr["mask2"]
    q = np.matmul(K, R.dot(X) + T)
    pixel_coord = q[:2, valid_idx] / q[-1:, valid_idx]                                               # :394
    trans3d = torch.eye(4)                                                                           # :430 with sc = 1, float32
    Kinv, rays = _rays(K, depth_curr, W, H)
    bx, by = round_coord[0, border_valid_idx], round_coord[1, border_valid_idx]
    with torch.no_grad():                                                                            # :442-447
        tr = _apply(trans3d, _world32(R, T, torch.matmul(Kinv, rays[:, by, bx].reshape(3, -1)))).numpy()
    trans3d = trans3d.numpy()
    Rinv = np.linalg.inv(R)
    hole = np.where(1 - mask2.reshape(-1))[0]
    origin = -Rinv.dot(T).astype(np.float32)                                                         # :452
    to_cam = tr - origin                                                                             # :459
    to_pcd = X[:, valid_idx[border_valid_idx]] - origin                                              # :460
    coeff = np.sum(to_pcd * to_cam, axis=0) / np.sum(to_cam * to_cam, axis=0)                        # :462
    foot = origin + to_cam * coeff.reshape(1, -1)                                                    # :463
    comp_corr = (R.dot(foot) + T)[-1] - (R.dot(tr) + T)[-1]                                          # :465-468
    compensate_depth = np.concatenate((comp_corr, np.zeros(4)), axis=0)                              # :469-470
    corners = np.array([[0, 0, W - 1, W - 1], [0, H - 1, 0, H - 1]])
    pixel_cam2 = np.concatenate((pixel_coord[:, border_valid_idx], corners), axis=1).transpose(1, 0)  # :472-474
    masked_xy = np.stack(np.where(1 - mask2), axis=1)[:, [1, 0]]                                     # :477
    lin = interp_grid(pixel_cam2, compensate_depth, masked_xy)                                       # :478
    near = interp_grid(pixel_cam2, compensate_depth, masked_xy, method="nearest")
    new_depth = np.where(np.isnan(lin), near, lin)                                                   # :479
    Kinv_np = np.linalg.inv(K)
    cam2 = np.matmul(Kinv_np, np.stack((x * depth_curr, y * depth_curr, 1 * depth_curr), axis=0).reshape(3, -1))[:, hole]
    xn, yn = x.reshape(-1)[hole], y.reshape(-1)[hole]
    comp_cam2 = np.matmul(Kinv_np, np.stack((xn * new_depth, yn * new_depth, 1 * new_depth), axis=0))            # :483
    world = (Rinv.dot(cam2 + comp_cam2) - Rinv.dot(T)).astype(np.float32)                            # :484-486
    world = np.matmul(trans3d, np.concatenate((world, np.ones((1, world.shape[1]))), axis=0))
    world = world[:3] / world[-1]                                                                    # :487-489
    colors = (np.array(image_curr).reshape(-1, 3).astype(np.float32) / 255.)[hole]                  # :490
    return dict(pixel_cam2=pixel_cam2, compensate_depth=compensate_depth, new_depth=new_depth.astype(np.float64),
                new_points=world.astype(np.float32), new_colors=colors, hole=hole.astype(np.int64))


def lifted_view(rng, H, W, K):
    """The cloud the reference starts from (:370-371): a wall 4..5 away with a box 2 away in front, lifted at the first pose."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    depth = (4.0 + x / W).astype(np.float32)
    box = (x > 0.35 * W) & (x < 0.65 * W) & (y > 0.3 * H) & (y < 0.8 * H)
    depth[box] = 2.0
    depth += rng.uniform(0, 0.003, depth.shape).astype(np.float32)       # off the rounding ties of an exact grid
    R0, T0 = pose(rng)
    cam = np.matmul(np.linalg.inv(K), np.stack((x * depth, y * depth, 1 * depth), axis=0).reshape(3, -1))
    X = (np.linalg.inv(R0).dot(cam) - np.linalg.inv(R0).dot(T0)).astype(np.float32)
    C = rng.random((H * W, 3)).astype(np.float32)
    return X, C, R0, T0


def two_layers(rng, N, H, W, K):
    R, T = pose(rng)
    u = np.concatenate([rng.uniform(-6, 0.68 * W, N - 25), rng.uniform(0.7 * W, W + 4, 25)])
    v = rng.uniform(-6, H + 5, N)
    z = np.where(rng.random(N) < 0.5, rng.uniform(2.8, 3.2, N), rng.uniform(5.5, 6.5, N))
    cam = np.linalg.inv(K) @ np.stack([u * z, v * z, z])
    X = (np.linalg.inv(R) @ (cam - T)).astype(np.float32)
    return X, rng.random((N, 3)).astype(np.float32), R, T


def network_depth(rng, H, W, base, scale):
    """The stand-in for the depth network: a smooth map near `base`, off by a scale, float32 as infer_pil returns it."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    d = (base + 0.4 * np.sin(x / W * 3.0) + 0.3 * np.cos(y / H * 2.0)) / scale
    return (d + rng.uniform(0, 0.002, d.shape)).astype(np.float32)


def main():
    rng = np.random.default_rng(20240923)
    H, W = 48, 64
    K = np.array([[58, 0, 32], [0, 58, 24], [0, 0, 1]], dtype=np.float32)          # exact in float32: see the module docstring
    out = {}
    for name in ("a", "b"):
        if name == "a":
            X, C, R0, T0 = lifted_view(rng, H, W, K.astype(np.float64))
            a = 0.12
            R = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]]) @ R0
            T = T0 + np.array([[-0.45], [0.02], [0.03]])
            depth_curr = network_depth(rng, H, W, 4.3, 1.07)
        else:
            X, C, R, T = two_layers(rng, 3000, H, W, K.astype(np.float64))
            depth_curr = network_depth(rng, H, W, 3.6, 0.93)
        fr = reference_frame(X, C, K.astype(np.float64), R, T, H, W)
        assert 0 < fr["mask2"].sum() < H * W and fr["border_valid_idx"].size > 20
        image_curr = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        if name == "a":
            sc, had_grad = adam_scale(K, R, T, H, W, depth_curr, fr["round_coord"], fr["valid_idx"], X)
            assert sc == 1.0 and not had_grad, (sc, had_grad)
            out["a_adam_scale"] = np.array([sc])
        ref = reference_dream(X, K, R, T, H, W, depth_curr, image_curr, fr)
        assert ref["hole"].size == int((fr["mask2"] == 0).sum()) and np.isfinite(ref["compensate_depth"]).all()
        out.update({f"{name}_{k}": v for k, v in dict(X=X, C=C, K=K.astype(np.float64), R=R, T=T, HW=np.array([H, W]),
                                                      depth=depth_curr, image=image_curr).items()})
        out.update({f"{name}_{k}": v for k, v in fr.items() if k in ("valid_idx", "round_coord", "border_valid_idx", "mask2",
                                                                     "mask_hf")})
        out.update({f"{name}_{k}": v for k, v in ref.items()})
        print(name, "N", X.shape[1], "valid", fr["valid_idx"].size, "border correspondences", fr["border_valid_idx"].size,
              "hole pixels", ref["hole"].size, "compensate_depth", ref["compensate_depth"].min(), ref["compensate_depth"].max())
    path = os.path.join(HERE, "ref_dream_fixtures.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
