"""Cost of the mesh clean-up (luciddreamer_amd.mesh.post_process) against the host route users take without it.

    python tools/mesh_bench.py [--dim 256] [--blobs 300] [--keep 50] [--min-faces 50] [--steps 12] [--warmup 2] [--commit SHA]
                               [--out profiles/mesh_bench.json]

Scene: a --dim^3 TSDF volume filled on the device with one large sphere and --blobs seeded small ones (floaters), extracted with
TSDFVolume.extract_mesh (timed once, for scale).  Then
  device : mesh.post_process(vertices, colors, faces, keep, min_faces, drop_degenerate=True): the cluster filter (its one
           synchronisation included) and the vertex normals of the cleaned mesh.
  host   : the same mesh copied to the host, connected components with SciPy (tests/mesh_ref.py's numpy labelling when SciPy is
           absent; "host_components" records which), numpy masks, re-indexing and normals, the result copied back.
Before any time is reported the two results are compared (faces and vertices exact, normals to the bit: a sanity check of the
partner, not a bar).  Both sides are timed with a host clock around the call and a device synchronise, ALTERNATING call by call;
medians, minima and every single run are kept; the device side is then timed the same way call after call without the partner in
between ("device_alone").  The three device calls are also timed one by one with HIP events; the labelling
pass is reported with the bytes of the face array it reads over its time.  Nothing is asserted about speed.  Prints ONE JSON line
and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import mesh_ref as MR  # noqa: E402

try:
    import scipy.sparse as _sp
    from scipy.sparse.csgraph import connected_components as _sp_components
except ImportError:                  # the numpy labelling of the restatement takes its place
    _sp = None


def fill_volume(vol, n_blobs, seed):
    """One large sphere and n_blobs small ones: signed distance / trunc clamped to [-1, 1], weight 1, a colour ramp.  The small
    spheres touch only their own boxes of the lattice."""
    nx, ny, nz = vol.dims
    dev, s = vol.device, vol.voxel_size
    ax = [torch.arange(n, device=dev, dtype=torch.float32) * s + o for n, o in zip((nx, ny, nz), vol.origin)]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    ext = [n * s for n in (nx, ny, nz)]
    centre = [o + 0.5 * e for o, e in zip(vol.origin, ext)]
    f = torch.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - 0.3 * min(ext)
    rng = np.random.default_rng(seed)
    for _ in range(n_blobs):
        r = float(rng.uniform(1.5, 6.0)) * s
        c = [o + float(rng.uniform(0.05, 0.95)) * e for o, e in zip(vol.origin, ext)]
        pad = r + vol.trunc + s
        lo = [max(0, int((c[k] - pad - vol.origin[k]) / s)) for k in range(3)]
        hi = [min(n, int((c[k] + pad - vol.origin[k]) / s) + 2) for k, n in enumerate((nx, ny, nz))]
        box = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
        d = torch.sqrt((x[box] - c[0]) ** 2 + (y[box] - c[1]) ** 2 + (z[box] - c[2]) ** 2) - r
        f[box] = torch.minimum(f[box], d)
    vol.tsdf.copy_(torch.clamp(f / vol.trunc, -1.0, 1.0))
    vol.weight.fill_(1.0)
    vol.color.copy_(torch.stack([(x - vol.origin[0]) / ext[0], (y - vol.origin[1]) / ext[1], (z - vol.origin[2]) / ext[2]], dim=-1))


def host_route(V, C, F, keep, min_faces):
    """What a user does today: copy, label, mask, re-index, normals, copy back."""
    dev = V.device
    v, c, f = V.cpu().numpy(), C.cpu().numpy(), F.cpu().numpy()
    nV = len(v)
    if _sp is not None:
        g = f.astype(np.int64)
        rows, cols = np.concatenate([g[:, 0], g[:, 0]]), np.concatenate([g[:, 1], g[:, 2]])
        n_comp, comp = _sp_components(_sp.coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(nV, nV)),
                                      directed=False)
        face_comp = comp[g[:, 0]]
        counts = np.bincount(face_comp, minlength=n_comp)
    else:
        face_comp, _, counts = MR.components(f, nV)
    thr = MR.threshold(counts, keep, min_faces)
    _, L = MR.face_cross(v, f)
    ok = (counts[face_comp] >= thr) & np.isfinite(L) & (L > 0) & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])
    used = np.zeros(nV, dtype=bool)
    used[f[ok].reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    v2, c2, f2 = v[used], c[used], new_id[f[ok]].astype(np.int32)
    n2 = MR.vertex_normals(v2, f2)
    return tuple(torch.from_numpy(a).to(dev) for a in (v2, c2, f2, n2)) + (int((counts > 0).sum()),)


def _clock_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _med(runs):
    return round(statistics.median(runs), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--blobs", type=int, default=300)
    ap.add_argument("--keep", type=int, default=50)
    ap.add_argument("--min-faces", type=int, default=50)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="", help="the commit the tree was made from (the measuring box has no .git)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    from luciddreamer_amd import _lib, mesh, tsdf

    n = args.dim
    s = 2.4 / n
    vol = tsdf.TSDFVolume((-1.2 + 0.013, -1.2 + 0.007, -1.2 + 0.011), s, (n, n, n), 4.0 * s, dev)
    fill_volume(vol, args.blobs, seed=7)
    vol.extract_mesh()                                              # warm-up
    extract_ms, (V, C, F) = _clock_ms(vol.extract_mesh)
    nV, nT = int(V.shape[0]), int(F.shape[0])

    device = lambda: mesh.post_process(V, C, F, keep_largest=args.keep, min_faces=args.min_faces, drop_degenerate=True)
    host = lambda: host_route(V, C, F, args.keep, args.min_faces)

    # the same mesh from both, before any time is reported
    dV, dC, dF, dN = device()
    hV, hC, hF, hN, n_components = host()
    faces_equal, vertices_equal = bool(torch.equal(dF, hF)), bool(torch.equal(dV, hV) and torch.equal(dC, hC))
    normals_equal = bool(torch.equal(dN.view(torch.int32), hN.view(torch.int32)))
    assert faces_equal and vertices_equal and normals_equal, (faces_equal, vertices_equal, normals_equal)

    runs = {"device": [], "host": []}
    for k in range(args.warmup + args.steps):
        a, _ = _clock_ms(device)
        b, _ = _clock_ms(host)
        if k >= args.warmup:
            runs["device"].append(a)
            runs["host"].append(b)

    # the device side alone, call after call: what the alternation with a host-heavy partner adds to it shows in the difference
    alone = []
    for k in range(args.warmup + args.steps):
        a, _ = _clock_ms(device)
        if k >= args.warmup:
            alone.append(a)

    # the three device calls one by one
    parts = {"components": [], "filter": [], "normals": []}
    for k in range(args.warmup + args.steps):
        a = _event_ms(lambda: mesh._components(F, nV))
        b = _event_ms(lambda: mesh.filter_clusters(V, F, colors=C, keep_largest=args.keep, min_faces=args.min_faces,
                                                   drop_degenerate=True))
        c = _event_ms(lambda: mesh.vertex_normals(dV, dF))
        if k >= args.warmup:
            for name, v in zip(parts, (a, b, c)):
                parts[name].append(v)

    dm, hm = _med(runs["device"]), _med(runs["host"])
    comp_ms = _med(parts["components"])
    res = {"tool": "mesh_bench", "box": torch.cuda.get_device_name(0), "version": _lib.lib().lr_version().decode(),
           "commits": {"tree_made_from": args.commit, "library_source_hash": _lib.lib().lr_version().decode().split()[-1]},
           "dims": [n, n, n], "blobs": args.blobs, "keep_largest": args.keep, "min_faces": args.min_faces,
           "steps": args.steps, "warmup": args.warmup, "order": "device, host, device, host, ... in one process",
           "timing": "host clock around the call and a device synchronise (post_process synchronises once itself); parts: HIP "
                     "events around each call, host launch and allocation included",
           "host_components": "scipy.sparse.csgraph.connected_components" if _sp is not None else "tests/mesh_ref.components",
           "n_vertices": nV, "n_faces": nT, "n_components": n_components,
           "n_vertices_kept": int(dV.shape[0]), "n_faces_kept": int(dF.shape[0]),
           "extract_mesh_ms_once": round(extract_ms, 4),
           "device_median_ms": dm, "host_median_ms": hm, "host_over_device": round(hm / dm, 2),
           "device_min_ms": round(min(runs["device"]), 4), "host_min_ms": round(min(runs["host"]), 4),
           "device_alone_median_ms": _med(alone), "host_over_device_alone": round(hm / _med(alone), 2),
           "faces_equal": faces_equal, "vertices_equal": vertices_equal, "normals_equal_bits": normals_equal,
           "parts_median_ms": {k: _med(v) for k, v in parts.items()},
           "components_face_bytes": nT * 12, "components_face_bytes_per_s": round(nT * 12 / (comp_ms * 1e-3), 0),
           "workspace_bytes": int(_lib.lib().lr_mesh_workspace_bytes(nV, nT)),
           "runs_ms": {k: [round(v, 4) for v in vs] for k, vs in {**runs, "device_alone": alone, **parts}.items()}}
    line = json.dumps(res, separators=(",", ":"))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
