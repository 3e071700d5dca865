"""Cost of TSDF integration and mesh extraction (luciddreamer_amd.tsdf) against the torch-op composition of the same definition.

    python tools/tsdf_bench.py [--dim 256] [--size 512] [--frames 8] [--steps 12] [--warmup 2] [--commit SHA]
                               [--out profiles/tsdf_bench.json]

Scene: eight analytic views (a sphere in front of a backdrop, tests/tsdf_cases.render_depth) of --size x --size pixels fused into
a --dim^3 volume around the sphere, with colour.
  integrate : TSDFVolume.integrate_batch (one launch for the eight frames) against torch_integrate below: the float64 projection,
              the gathers and the running mean as about twenty torch ops per frame over the [N] lattice.
  extract   : TSDFVolume.extract_mesh (count + emit, its one synchronisation included) against torch_extract below: the six
              tetrahedra of every cell through a lookup table, torch.unique for the welding.
Before any time is reported the two sides are compared (touched set and faces exact, values to 1e-5; a sanity check of the
partner, not a bar).  Each call is timed with HIP events (extract: a host clock around the call, which ends in its own
synchronise; the composition is synchronised the same way), fused and composition ALTERNATING call by call; medians, minima and
every single run are kept.  Compulsory bytes of the integration: D, W and colour of every voxel read once (20 B), written once
for a touched voxel (20 B), and every pixel's depth and colour read once (16 B per pixel and frame; the per-voxel gathers of them
are cache hits beyond that).  Nothing is asserted about
speed.  Prints ONE JSON line and writes it to --out.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import tsdf_cases as TC  # noqa: E402
from tests import tsdf_ref as TR  # noqa: E402

HBM_ACHIEVABLE = 6.3e12             # B/s


def torch_integrate(D, Wt, C, X, depths, colors, K, Rs, Ts, trunc):
    """The definition of lr_tsdf_integrate in torch ops (no pixel weights, no limits): D, Wt [N], C [N,3], X [N,3] float32."""
    F, H, W = depths.shape
    x, y, z = X[:, 0].double(), X[:, 1].double(), X[:, 2].double()
    row = lambda m, a, b, c: (m[0] * a + m[1] * b) + m[2] * c
    for f in range(F):
        R, T = Rs[f], Ts[f]
        p = [row(R[i], x, y, z) + T[i] for i in range(3)]
        q = [row(K[i], p[0], p[1], p[2]) for i in range(3)]
        u, v = q[0] / q[2], q[1] / q[2]
        valid = (q[2] > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        pix = torch.where(valid, torch.round(v) * W + torch.round(u), torch.zeros_like(u)).long()
        d = depths[f].reshape(-1)[pix]
        sdf = d - q[2].float()
        ok = valid & torch.isfinite(d) & (d > 0) & ~(sdf < -trunc)
        val = torch.clamp(sdf / trunc, max=1.0)
        Wn = Wt + 1.0
        D = torch.where(ok, (D * Wt + val) / Wn, D)
        c = colors[f].reshape(-1, 3)[pix]
        C = torch.where(ok[:, None], (C * Wt[:, None] + c) / Wn[:, None], C)
        Wt = torch.where(ok, Wn, Wt)
    return D, Wt, C


class TorchExtract:
    """The definition of lr_tsdf_extract_* in torch ops; the triangle table is the restatement's (tests/tsdf_ref.TRIANGLES)."""

    def __init__(self, dims, origin, s, dev):
        nx, ny, nz = dims
        self.dims, self.s, self.dev = dims, s, dev
        self.origin = torch.tensor(origin, dtype=torch.float32, device=dev)
        nxy = nx * ny
        lin = lambda v: v[0] + v[1] * nx + v[2] * nxy
        tets = [TR.tet_vertices(t) for t in range(6)]
        self.voff = torch.tensor([[lin(v) for v in tets[t]] for t in range(6)], device=dev)                         # [6,4]
        table = np.full((6, 16, 2, 3, 2), -1, dtype=np.int64)
        for t in range(6):
            for m in range(16):
                for k, tri in enumerate(TR.TRIANGLES[t][m]):
                    table[t, m, k] = tri
        self.table = torch.from_numpy(table).to(dev)
        dirs = np.zeros((6, 4, 4), dtype=np.int64)
        for t in range(6):
            for lo in range(4):
                for hi in range(lo + 1, 4):
                    dirs[t, lo, hi] = TR.DIRS.index(tuple(tets[t][hi][c] - tets[t][lo][c] for c in range(3)))
        self.dirs = torch.from_numpy(dirs).to(dev)
        self.dvec = torch.tensor(TR.DIRS, device=dev)
        k, j, i = torch.meshgrid(torch.arange(nz - 1, device=dev), torch.arange(ny - 1, device=dev),
                                 torch.arange(nx - 1, device=dev), indexing="ij")
        self.cells = ((k * ny + j) * nx + i).reshape(-1)                                                            # ascending
        self.corner = torch.tensor([lin((c & 1, (c >> 1) & 1, c >> 2)) for c in range(8)], device=dev)

    def __call__(self, tsdf, weight, color, min_weight=1.0):
        nx, ny, nz = self.dims
        nxy = nx * ny
        D, Wt, C = tsdf.reshape(-1), weight.reshape(-1), color.reshape(-1, 3)
        inside = D < 0
        corner = self.cells[:, None] + self.corner[None]                              # [cells, 8]
        n_in = inside[corner].sum(dim=1)
        keep = (Wt[corner] >= min_weight).all(dim=1) & (n_in > 0) & (n_in < 8)
        g = self.cells[keep]                                                          # [n]
        vert = g[:, None, None] + self.voff[None]                                     # [n,6,4]
        m = (inside[vert].long() << torch.arange(4, device=self.dev)).sum(dim=2)      # [n,6]
        tri = self.table[torch.arange(6, device=self.dev)[None], m]                   # [n,6,2,3,2]
        live = tri[..., 0, 0] >= 0                                                    # [n,6,2]
        lo, hi = tri[..., 0].clamp(min=0), tri[..., 1].clamp(min=0)                   # [n,6,2,3]
        t_idx = torch.arange(6, device=self.dev)[None, :, None, None].expand_as(lo)
        lower = torch.gather(vert[:, :, None, :].expand(-1, -1, 2, -1), 3, lo)        # lattice point of the lower end
        ids = (7 * lower + self.dirs[t_idx, lo, hi])[live]                            # [T,3], cell, tetrahedron, triangle order
        uniq, inverse = torch.unique(ids, return_inverse=True)
        p, d = uniq // 7, uniq % 7
        dv = self.dvec[d]
        q = p + dv[:, 0] + dv[:, 1] * nx + dv[:, 2] * nxy
        ijk = torch.stack([p % nx, (p // nx) % ny, p // nxy], dim=1)
        t = D[p] / (D[p] - D[q])
        cp = ijk.float() * self.s + self.origin
        cq = (ijk + dv).float() * self.s + self.origin
        return cp + t[:, None] * (cq - cp), C[p] + t[:, None] * (C[q] - C[p]), inverse.to(torch.int32)


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _clock_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _summary(runs):
    f, c = runs["fused"], runs["composition"]
    return {"fused_median_ms": round(statistics.median(f), 4), "composition_median_ms": round(statistics.median(c), 4),
            "composition_over_fused": round(statistics.median(c) / statistics.median(f), 2),
            "fused_min_ms": round(min(f), 4), "composition_min_ms": round(min(c), 4),
            "runs_ms": {k: [round(v, 4) for v in vs] for k, vs in runs.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="", help="the commit the tree was made from (the measuring box has no .git)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_bench: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib, tsdf

    n, S, F = args.dim, args.size, args.frames
    s = 2.4 / n
    origin = (-1.2 + 0.013, -1.2 + 0.007, -1.2 + 0.011)
    trunc = 4.0 * s
    K = np.array([[0.8 * S, 0.0, (S - 1) / 2.0], [0.0, 0.8 * S, (S - 1) / 2.0], [0.0, 0.0, 1.0]])
    poses = [(2.0 * math.pi * f / F, 0.3 * math.sin(1.7 * f), 0.0, (0.0, 0.0, 0.0)) for f in range(F)]
    Rs, Ts = [], []
    for yaw, pitch, roll, _ in poses:                              # on a circle of radius 3 around the sphere, looking at it
        c2w = TC.posed_cases.c2w_of((yaw, pitch, roll, (0.0, 0.0, 0.0)))
        c2w[:3, 3] = c2w[:3, :3] @ np.array([0.0, 0.0, -3.0])
        w2c = np.linalg.inv(c2w)
        Rs.append(w2c[:3, :3])
        Ts.append(w2c[:3, 3])
    Rs, Ts = np.ascontiguousarray(np.stack(Rs)), np.ascontiguousarray(np.stack(Ts))
    depths = np.stack([TC.render_depth(K, R, T, S, S, (0.02, -0.03, 0.01), 0.8, 1e9) for R, T in zip(Rs, Ts)])
    depths[depths > 100.0] = 8.0
    depths = torch.from_numpy(depths).to(dev)
    colors = torch.rand((F, S, S, 3), generator=torch.Generator().manual_seed(1)).to(dev)

    vol = tsdf.TSDFVolume(origin, s, (n, n, n), trunc, dev)
    ref = TR.RefVolume(origin, s, (n, n, n), trunc)
    X = torch.from_numpy(ref.lattice()).to(dev)
    Kt, Rt, Tt = (torch.from_numpy(a).to(dev) for a in (K, Rs, Ts))
    N = n ** 3

    def fused_integrate():
        vol.integrate_batch(depths, K, Rs, Ts, colors=colors)

    state = {}

    def comp_integrate():
        state["out"] = torch_integrate(torch.ones(N, device=dev), torch.zeros(N, device=dev), torch.zeros((N, 3), device=dev), X,
                                       depths, colors, Kt, Rt, Tt, trunc)

    # the same volume from both, before any time is reported
    vol.reset()
    fused_integrate()
    comp_integrate()
    D, Wt, C = state["out"]
    touched_equal = bool(torch.equal(vol.weight.reshape(-1) > 0, Wt > 0))
    tsdf_diff = float((vol.tsdf.reshape(-1) - D).abs().max())
    color_diff = float((vol.color.reshape(-1, 3) - C).abs().max())
    assert touched_equal and tsdf_diff <= 1e-5 and color_diff <= 1e-5, (touched_equal, tsdf_diff, color_diff)

    runs_i = {"fused": [], "composition": []}
    for k in range(args.warmup + args.steps):
        vol.reset()
        a = _event_ms(fused_integrate)
        b = _event_ms(comp_integrate)
        if k >= args.warmup:
            runs_i["fused"].append(a)
            runs_i["composition"].append(b)
    state.clear()

    vol.reset()
    fused_integrate()
    extractor = TorchExtract((n, n, n), origin, s, dev)
    V, Cv, Fc = vol.extract_mesh()
    V2, C2, F2 = extractor(vol.tsdf, vol.weight, vol.color)
    faces_equal = bool(torch.equal(Fc, F2))
    vert_diff = float((V - V2).abs().max())
    assert faces_equal and vert_diff <= 1e-5 and float((Cv - C2).abs().max()) <= 1e-5, (faces_equal, vert_diff)
    runs_e = {"fused": [], "composition": []}
    for k in range(args.warmup + args.steps):
        a = _clock_ms(lambda: vol.extract_mesh())
        b = _clock_ms(lambda: extractor(vol.tsdf, vol.weight, vol.color))
        if k >= args.warmup:
            runs_e["fused"].append(a)
            runs_e["composition"].append(b)

    n_touched = int((vol.weight > 0).sum())
    bytes_needed = N * 20 + n_touched * 20 + F * S * S * 16
    integ, extr = _summary(runs_i), _summary(runs_e)
    integ.update(n_touched=n_touched, bytes_needed=bytes_needed, fused_bytes_per_s=round(bytes_needed / (integ["fused_median_ms"] * 1e-3), 0),
                 share_of_achievable_hbm=round(bytes_needed / (integ["fused_median_ms"] * 1e-3) / HBM_ACHIEVABLE, 4),
                 touched_equal=touched_equal, max_tsdf_difference=tsdf_diff, max_color_difference=color_diff)
    extr.update(n_vertices=int(V.shape[0]), n_faces=int(Fc.shape[0]), faces_equal=faces_equal, max_vertex_difference=vert_diff,
                workspace_bytes=int(_lib.lib().lr_tsdf_workspace_bytes(_lib.TsdfExtractArgs(vol=vol._desc()))))
    res = {"tool": "tsdf_bench", "box": torch.cuda.get_device_name(0), "version": _lib.lib().lr_version().decode(),
           "commits": {"tree_made_from": args.commit, "library_source_hash": _lib.lib().lr_version().decode().split()[-1]},
           "dims": [n, n, n], "frames": F, "frame_size": [S, S], "steps": args.steps, "warmup": args.warmup,
           "order": "fused, composition, fused, composition, ... in one process",
           "timing": "integrate: HIP events around the call, host launch included; extract: host clock around the call and a "
                     "device synchronise (extract_mesh synchronises once itself)",
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "integrate": integ, "extract": extr}
    line = json.dumps(res, separators=(",", ":"))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
