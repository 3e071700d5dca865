"""Seeded cases of the mesh clean-up tests (test helper, not collected): the meshes of tsdf_cases.field_mesh, the `blobs` field
(six spheres of different sizes), and index-only meshes -- a shuffled strip, a strip in vertex order, a forest of single faces, a fan, a mixed mesh with
every kind of bad face.  Shared by tests/test_mesh_cpu.py and tests/test_gpu_mesh.py; references are computed once per process
(functools.lru_cache) and callers do not modify them."""
import functools

import numpy as np

from tests import mesh_ref, tsdf_cases, tsdf_ref

# ---- blobs: the union of six spheres in a 40 x 32 x 24 volume, s = 1, trunc = 3, weight 1 ---------------------------------------
BLOBS_DIMS, BLOBS_S, BLOBS_TRUNC = (40, 32, 24), 1.0, 3.0
BLOBS = (((10.3, 12.6, 11.45), 7.2), ((26.4, 8.3, 7.6), 3.1), ((26.4, 22.3, 14.6), 3.1), ((34.5, 15.45, 6.4), 2.05),
         ((33.3, 26.6, 18.5), 1.2), ((21.0, 27.0, 20.0), 0.4))
# what tsdf_ref gives: face counts by size, the labels in that order, and the sizes of the mesh.  The two radius-3.1 spheres are
# lattice translates of each other: they tie.
BLOBS_COUNTS = (5772, 1072, 1072, 408, 144, 24)
BLOBS_LABELS = (30, 0, 2246, 156, 4014, 4218)
BLOBS_V, BLOBS_T = 4258, 8492

FIELD_NAMES = tsdf_cases.FIELD_NAMES + ("blobs",)
# faces of zero area (exact zeros of the field) and the number of components
FIELD_FACTS = {"sphere": (0, 1), "torus": (0, 1), "plane": (0, 1), "wide": (0, 1), "sphere_zeroed": (1732, 1), "thin": (223, 29),
               "empty": (0, 0), "blobs": (52, 6)}
THIN_LARGEST = (560, 348, 320, 220, 196)


@functools.lru_cache(maxsize=None)
def blobs_field():
    vol = tsdf_ref.RefVolume((0.0, 0.0, 0.0), BLOBS_S, BLOBS_DIMS, BLOBS_TRUNC)
    x, y, z = tsdf_cases._grid(BLOBS_DIMS)
    f = np.full(x.shape, np.inf)
    for c, r in BLOBS:
        f = np.minimum(f, np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r)
    vol.tsdf = np.clip(f / BLOBS_TRUNC, -1.0, 1.0).astype(np.float32)
    vol.weight = np.ones(x.shape, dtype=np.float32)
    vol.color = tsdf_cases._colors(x, y, z, BLOBS_DIMS)
    return vol


@functools.lru_cache(maxsize=None)
def field_mesh(name):
    """(vertices, colors, faces) of the restatement: tsdf_cases' fields and `blobs`."""
    return blobs_field().extract(1.0) if name == "blobs" else tsdf_cases.field_mesh(name)


# ---- index-only meshes ------------------------------------------------------------------------------------------------------------
def _positions(rng, n):
    return rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def synthetic(name):
    """(vertices [V,3] float32, faces [T,3] int32)."""
    if name in ("strip", "long_strip"):
        # faces[i] = (p[i], p[i+1], p[i+2]) over a permutation p, rows shuffled: one component; a label travels thousands of
        # hops, across workgroups.  long_strip: more than 256 scan tiles of 2048 rows, a second round of the block-sum scan
        T = 5000 if name == "strip" else 530000
        rng = np.random.default_rng(T)
        p = rng.permutation(T + 2).astype(np.int32)
        faces = np.stack([p[:-2], p[1:-1], p[2:]], axis=1)[rng.permutation(T)]
        vertices = _positions(rng, T + 2)
    elif name == "ordered_strip":
        # the strip in vertex order, rows in order: concurrent hooking alone leaves the chain parent[k] = k - 1, as long as the
        # component, and walks over it are quadratic without path splitting
        T = 200000
        rng = np.random.default_rng(T)
        i = np.arange(T, dtype=np.int32)
        faces = np.stack([i, i + 1, i + 2], axis=1)
        vertices = _positions(rng, T + 2)
    elif name == "forest":
        # 3001 components of one face: T is no multiple of 64, 256 or 2048
        rng = np.random.default_rng(3001)
        faces = rng.permutation(3 * 3001).astype(np.int32).reshape(3001, 3)
        vertices = _positions(rng, 3 * 3001)
    elif name == "fan":
        # 3000 faces round vertex 7 (after the permutation): valence above 2048, which an int32 sum of 2^20 steps would overflow
        rng = np.random.default_rng(3000)
        rim = np.arange(1, 3001)
        faces = np.stack([np.zeros(3000, np.int64), rim, np.roll(rim, -1)], axis=1)
        p = rng.permutation(3001)
        p[[0, np.nonzero(p == 7)[0][0]]] = p[[np.nonzero(p == 7)[0][0], 0]]          # the hub becomes vertex 7
        faces = p[faces].astype(np.int32)[rng.permutation(3000)]
        vertices = _positions(rng, 3001)
    elif name == "mixed":
        # duplicate faces, repeated indices, indices -1, V and 2^31 - 1, unreferenced vertices, a NaN and a +inf coordinate
        rng = np.random.default_rng(77)
        V = 400
        vertices = _positions(rng, V)
        vertices[17, 1] = np.nan
        vertices[230, 0] = np.inf
        base = rng.integers(0, 300, size=(260, 3))                          # vertices 300.. stay unreferenced (but for below)
        base[:40] = np.sort(rng.integers(0, 300, size=(40, 1)) + np.array([[0, 1, 2]]), axis=1) % 300
        faces = np.concatenate([base, base[5:25], base[100:110, ::-1],     # duplicates, some with the other winding
                                np.stack([base[30:50, 0], base[30:50, 0], base[30:50, 2]], axis=1),     # a repeated index
                                np.stack([base[60:66, 1]] * 3, axis=1),                                 # three times the same
                                np.array([[-1, 3, 4], [5, V, 6], [7, 8, 2 ** 31 - 1], [-2 ** 31, 1, 2], [V - 1, V - 2, V - 3],
                                          [17, 18, 19], [230, 231, 232], [350, 351, 352], [350, 352, 353]])])
        faces = faces[rng.permutation(len(faces))].astype(np.int32)
    else:
        raise KeyError(name)
    vertices.setflags(write=False)
    faces.setflags(write=False)
    return vertices, faces


SYNTHETIC_NAMES = ("strip", "long_strip", "ordered_strip", "forest", "fan", "mixed")


def mesh(name):
    """(vertices, colors or None, faces) of any case."""
    if name in FIELD_NAMES:
        return field_mesh(name)
    v, f = synthetic(name)
    return v, None, f


ALL_NAMES = FIELD_NAMES + SYNTHETIC_NAMES


@functools.lru_cache(maxsize=None)
def components_reference(name):
    """(face_labels, vertex_labels, labels, counts) of the restatement."""
    v, _, f = mesh(name)
    out = mesh_ref.connected_components(f, len(v))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def normals_reference(name):
    v, _, f = mesh(name)
    out = mesh_ref.vertex_normals(v, f)
    out.setflags(write=False)
    return out


# (keep_largest, min_faces, drop_degenerate)
FILTER_SETTINGS = ((0, 1, False), (1, 1, False), (2, 1, False), (3, 1, False), (100, 1, False), (0, 100, False),
                   (2, 2000, False), (0, 10 ** 9, False), (0, 1, True))
FILTER_MESHES = ("blobs", "thin", "sphere_zeroed", "mixed")


@functools.lru_cache(maxsize=None)
def attribute_normals(name):
    """A seeded per-vertex attribute to travel through the filter as `normals`."""
    v, _, _ = mesh(name)
    out = np.random.default_rng(len(v)).normal(size=(len(v), 3)).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def filter_reference(name, setting):
    v, c, f = mesh(name)
    K, M, dd = setting
    return mesh_ref.filter_clusters(v, f, colors=c, normals=attribute_normals(name), keep_largest=K, min_faces=M,
                                    drop_degenerate=dd)
