"""Plain numpy restatement of luciddreamer_amd.tsdf (csrc/tsdf.hip), operation for operation (test helper, not collected).

Every float32 expression is written elementwise on float32 arrays in the order the header documents (include/lucid_raster.h,
lr_tsdf_*), so numpy forms the same bits as the device; the projection is tests/reproject_ref.project_points (float64).

    RefVolume(origin, voxel_size, dims, trunc, max_weight=inf)     .tsdf / .weight / .color numpy arrays, [nz,ny,nx(,3)]
        .integrate(depths [F,H,W], K, Rs, Ts, colors=None, pixel_weights=None, depth_max=inf) -> touched [nz,ny,nx] bool
        .extract(min_weight=1.0) -> (vertices [V,3] float32, colors [V,3] float32, faces [T,3] int32)
    TRIANGLES[t][m]    the triangles of tetrahedron t under inside mask m, each a triple of (lower, upper) tetrahedron vertices

The winding here is derived GEOMETRICALLY, once, from the unit cell: every vertex at its edge's midpoint, the normal must point
from the inside vertices to the outside ones (exact arithmetic on half-integers).  The kernel uses a closed form (permutation
parity and mask); the two derivations meet in the bit comparison of the faces.

Mesh checks shared by the CPU and GPU tests: directed_edges, is_closed, euler, open_edges."""
import itertools

import numpy as np

from tests import reproject_ref

DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))          # lexicographic


def tet_vertices(t):
    """The four corners (0/1 triples) of tetrahedron t: v0 = 0, v1 = e_a, v2 = e_a + e_b, v3 = (1,1,1)."""
    a, b, _ = PERMS[t]
    v1 = [0, 0, 0]
    v1[a] = 1
    v2 = list(v1)
    v2[b] = 1
    return ((0, 0, 0), tuple(v1), tuple(v2), (1, 1, 1))


def _edge(x, y):
    return (x, y) if x < y else (y, x)


def _tet_triangles(t, m):
    inside = [v for v in range(4) if (m >> v) & 1]
    outside = [v for v in range(4) if not (m >> v) & 1]
    if not inside or not outside:
        return ()
    if len(inside) == 2:
        p, q = inside
        r, s = outside
        tris = [(_edge(p, r), _edge(p, s), _edge(q, s)), (_edge(p, r), _edge(q, s), _edge(q, r))]
    else:
        l = inside[0] if len(inside) == 1 else outside[0]
        tris = [tuple(_edge(l, o) for o in range(4) if o != l)]
    V = np.array(tet_vertices(t), dtype=np.float64)
    toward = V[outside].mean(axis=0) - V[inside].mean(axis=0)
    out = []
    for tri in tris:
        mid = [(V[x] + V[y]) / 2 for x, y in tri]
        n = np.cross(mid[1] - mid[0], mid[2] - mid[0])
        side = float(np.dot(n, toward))
        assert side != 0.0, (t, m)
        out.append(tri if side > 0 else (tri[0], tri[2], tri[1]))
    return tuple(out)


TRIANGLES = tuple(tuple(_tet_triangles(t, m) for m in range(16)) for t in range(6))


class RefVolume:
    def __init__(self, origin, voxel_size, dims, trunc, max_weight=np.inf):
        self.origin = np.asarray(origin, dtype=np.float32)
        self.s = np.float32(voxel_size)
        self.dims = tuple(int(v) for v in dims)
        self.trunc = np.float32(trunc)
        self.max_weight = np.float32(max_weight)
        nx, ny, nz = self.dims
        self.tsdf = np.ones((nz, ny, nx), dtype=np.float32)
        self.weight = np.zeros((nz, ny, nx), dtype=np.float32)
        self.color = np.zeros((nz, ny, nx, 3), dtype=np.float32)

    def axis_coords(self, c):
        """float32(i) * s + origin_c: one multiply, then one add."""
        return np.arange(self.dims[c], dtype=np.float32) * self.s + self.origin[c]

    def lattice(self):
        """[N,3] float32 lattice points in linear order (x fastest)."""
        nx, ny, nz = self.dims
        x, y, z = self.axis_coords(0), self.axis_coords(1), self.axis_coords(2)
        X = np.empty((nz, ny, nx, 3), dtype=np.float32)
        X[..., 0] = x[None, None, :]
        X[..., 1] = y[None, :, None]
        X[..., 2] = z[:, None, None]
        return X.reshape(-1, 3)

    def integrate(self, depths, K, Rs, Ts, colors=None, pixel_weights=None, depth_max=np.inf):
        depths = np.asarray(depths, dtype=np.float32)
        F, H, W = depths.shape
        Rs = np.asarray(Rs, dtype=np.float64).reshape(F, 3, 3)
        Ts = np.asarray(Ts, dtype=np.float64).reshape(F, 3)
        X = self.lattice()
        D, Wt = self.tsdf.reshape(-1).copy(), self.weight.reshape(-1).copy()
        C = self.color.reshape(-1, 3).copy()
        touched = np.zeros(D.shape, dtype=bool)
        one = np.float32(1)
        for f in range(F):
            valid, iu, iv, _, _, z32, _ = reproject_ref.project_points(X, K, Rs[f], Ts[f], H, W)
            with np.errstate(all="ignore"):
                d = depths[f][iv, iu]
                ok = valid & np.isfinite(d) & (d > 0) & (d <= np.float32(depth_max))
                w = np.asarray(pixel_weights[f], dtype=np.float32)[iv, iu] if pixel_weights is not None else np.ones_like(d)
                ok &= np.isfinite(w) & (w > 0)
                sdf = d - z32
                ok &= ~(sdf < -self.trunc)
                v = np.minimum(one, sdf / self.trunc)
                Wn = Wt + w
                Dn = (D * Wt + v * w) / Wn
                D = np.where(ok, Dn, D)
                if colors is not None:
                    c = np.asarray(colors[f], dtype=np.float32)[iv, iu]
                    Cn = (C * Wt[:, None] + c * w[:, None]) / Wn[:, None]
                    C = np.where(ok[:, None], Cn, C)
                Wt = np.where(ok, np.minimum(Wn, self.max_weight), Wt)
            touched |= ok
        assert D.dtype == np.float32 and Wt.dtype == np.float32 and C.dtype == np.float32
        self.tsdf, self.weight = D.reshape(self.tsdf.shape), Wt.reshape(self.weight.shape)
        if colors is not None:
            self.color = C.reshape(self.color.shape)
        return touched.reshape(self.tsdf.shape)

    def extract(self, min_weight=1.0):
        nx, ny, nz = self.dims
        nxy = nx * ny
        D = self.tsdf.reshape(-1)
        inside = self.tsdf < 0
        with np.errstate(invalid="ignore"):
            good = self.weight >= np.float32(min_weight)
        corners = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
        sub = lambda a, c: a[c[2]:nz - 1 + c[2], c[1]:ny - 1 + c[1], c[0]:nx - 1 + c[0]]
        valid = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
        n_in = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int32)
        for c in corners:
            valid &= sub(good, c)
            n_in += sub(inside, c)
        cells = np.argwhere(valid & (n_in > 0) & (n_in < 8))         # (k, j, i), ascending linear index
        tets = [tet_vertices(t) for t in range(6)]
        tris = []
        for k, j, i in cells:
            g = (k * ny + j) * nx + i
            for t in range(6):
                vs = tets[t]
                lin = [g + v[0] + v[1] * nx + v[2] * nxy for v in vs]
                m = sum(1 << n for n in range(4) if D[lin[n]] < 0)
                for tri in TRIANGLES[t][m]:
                    ids = []
                    for lo, hi in tri:
                        d = tuple(vs[hi][c] - vs[lo][c] for c in range(3))
                        ids.append(7 * lin[lo] + DIRS.index(d))
                    tris.append(ids)
        tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
        ids = np.unique(tris)
        faces = np.searchsorted(ids, tris).astype(np.int32)
        p, d = ids // 7, ids % 7
        dvec = np.asarray(DIRS, dtype=np.int64)[d] if ids.size else np.zeros((0, 3), dtype=np.int64)
        q = p + dvec[:, 0] + dvec[:, 1] * nx + dvec[:, 2] * nxy
        ijk = np.stack([p % nx, (p // nx) % ny, p // nxy], axis=1)
        with np.errstate(all="ignore"):
            t = D[p] / (D[p] - D[q])
            V = np.empty((ids.size, 3), dtype=np.float32)
            for c in range(3):
                cp = ijk[:, c].astype(np.float32) * self.s + self.origin[c]
                cq = (ijk[:, c] + dvec[:, c]).astype(np.float32) * self.s + self.origin[c]
                V[:, c] = cp + t * (cq - cp)
            K = self.color.reshape(-1, 3)
            Cv = K[p] + t[:, None] * (K[q] - K[p])
        assert t.dtype == np.float32 and Cv.dtype == np.float32
        return V, Cv.astype(np.float32), faces


# ---- mesh checks ---------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    """{(a, b): count} over the three directed edges of every face."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
    out = {}
    for a, b in map(tuple, e):
        out[(a, b)] = out.get((a, b), 0) + 1
    return out


def open_edges(faces):
    """The directed edges whose reverse does not occur."""
    de = directed_edges(faces)
    return [e for e in de if (e[1], e[0]) not in de]


def is_closed(faces):
    """Every directed edge occurs once and its reverse once: a closed, consistently oriented surface."""
    de = directed_edges(faces)
    return len(de) > 0 and all(n == 1 and de.get((b, a), 0) == 1 for (a, b), n in de.items())


def euler(n_vertices, faces):
    """V - E + F with E the undirected edges."""
    de = directed_edges(faces)
    E = len({(min(a, b), max(a, b)) for a, b in de})
    return int(n_vertices) - E + int(np.asarray(faces).reshape(-1, 3).shape[0])


def all_referenced(n_vertices, faces):
    return np.array_equal(np.unique(np.asarray(faces)), np.arange(int(n_vertices)))
