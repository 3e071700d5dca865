"""numpy restatement of the mesh clean-up definitions of include/lucid_raster.h (lr_mesh_*): connected components, the cluster
filter and vertex normals (test helper, not collected; numpy only).  Every float64 operation is one numpy operation in the
header's order, so the device must give the same bits."""
import numpy as np

NORMAL_SCALE = 1048576.0          # 2^20


def in_range(faces, n_vertices):
    """[T] bool: every index of the face lies in [0, n_vertices)."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    return ((f >= 0) & (f < n_vertices)).all(axis=1)


def components(faces, n_vertices):
    """(face_labels [T], vertex_labels [V], component_faces [V]) int32.  Vectorised hooking of every root onto the smallest root
    an edge joins it to, then pointer jumping, until no edge joins two roots."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V = int(n_vertices)
    ok = in_range(f, V)
    g = f[ok]
    u = np.concatenate([g[:, 0], g[:, 0]])
    w = np.concatenate([g[:, 1], g[:, 2]])
    parent = np.arange(V, dtype=np.int64)
    while True:
        ru, rw = parent[u], parent[w]
        m = ru != rw
        if not m.any():
            break
        u, w, ru, rw = u[m], w[m], ru[m], rw[m]                    # an edge inside one tree stays inside it
        np.minimum.at(parent, np.maximum(ru, rw), np.minimum(ru, rw))
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    vertex_labels = parent.astype(np.int32)
    face_labels = np.full(f.shape[0], -1, dtype=np.int32)
    face_labels[ok] = vertex_labels[g[:, 0]]
    component_faces = np.bincount(face_labels[ok], minlength=V).astype(np.int32)[:V] if V else np.zeros(0, np.int32)
    return face_labels, vertex_labels, component_faces


def connected_components(faces, n_vertices):
    """(face_labels, vertex_labels, labels [C] ascending, counts [C]) as mesh.connected_components."""
    face_labels, vertex_labels, component_faces = components(faces, n_vertices)
    labels = np.nonzero(component_faces)[0].astype(np.int32)
    return face_labels, vertex_labels, labels, component_faces[labels]


def face_cross(vertices, faces):
    """(n [T,3], L [T]) float64 of faces whose indices are all in range."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    with np.errstate(all="ignore"):
        a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
        e1, e2 = b - a, c - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return n, L


def threshold(component_faces, keep_largest, min_faces):
    c = np.sort(component_faces[component_faces > 0])[::-1]
    kth = int(c[keep_largest - 1]) if 1 <= keep_largest <= len(c) else 0
    return max(kth, int(min_faces))


def filter_clusters(vertices, faces, colors=None, normals=None, keep_largest=0, min_faces=1, drop_degenerate=False):
    """dict(vertices, faces, colors, normals, vertex_index, face_index) of the filtered mesh."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V = v.shape[0]
    face_labels, _, component_faces = components(f, V)
    ok = face_labels >= 0
    keep = ok.copy()
    keep[ok] = component_faces[face_labels[ok]] >= threshold(component_faces, keep_largest, min_faces)
    if drop_degenerate:
        g = f[keep]
        _, L = face_cross(v, g)
        good = (g[:, 0] != g[:, 1]) & (g[:, 0] != g[:, 2]) & (g[:, 1] != g[:, 2]) & np.isfinite(L) & (L > 0)
        keep[keep] = good
    used = np.zeros(V, dtype=bool)
    used[f[keep].reshape(-1)] = True
    vertex_index = np.nonzero(used)[0].astype(np.int32)
    face_index = np.nonzero(keep)[0].astype(np.int32)
    new_id = np.cumsum(used) - 1
    return dict(vertices=v[vertex_index], faces=new_id[f[face_index]].astype(np.int32).reshape(-1, 3),
                colors=None if colors is None else np.asarray(colors, np.float32).reshape(-1, 3)[vertex_index],
                normals=None if normals is None else np.asarray(normals, np.float32).reshape(-1, 3)[vertex_index],
                vertex_index=vertex_index, face_index=face_index)


def vertex_normals(vertices, faces):
    """[V,3] float32."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V = v.shape[0]
    g = f[in_range(f, V)]
    n, L = face_cross(v, g)
    good = np.isfinite(L) & (L > 0)
    g, n, L = g[good], n[good], L[good]
    q = np.rint(n / L[:, None] * NORMAL_SCALE).astype(np.int64)
    sums = np.zeros((V, 3), dtype=np.int64)
    for k in range(3):
        np.add.at(sums, g[:, k], q)
    s = sums.astype(np.float64)
    S = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    with np.errstate(all="ignore"):
        out = (s / S[:, None]).astype(np.float32)
    out[S == 0] = 0.0
    return out


def post_process(vertices, colors, faces, keep_largest=50, min_faces=50, drop_degenerate=True):
    """(vertices, colors, faces, normals) as mesh.post_process."""
    r = filter_clusters(vertices, faces, colors=colors, keep_largest=keep_largest, min_faces=min_faces,
                        drop_degenerate=drop_degenerate)
    return r["vertices"], r["colors"], r["faces"], vertex_normals(r["vertices"], r["faces"])


def component_euler(n_vertices, faces, face_labels, label):
    """V - E + F of the component `label` (its own vertices, undirected edges and faces)."""
    g = np.asarray(faces).reshape(-1, 3)[face_labels == label].astype(np.int64)
    e = np.sort(np.concatenate([g[:, [0, 1]], g[:, [1, 2]], g[:, [2, 0]]]), axis=1)
    return len(np.unique(g)) - len(np.unique(e, axis=0)) + len(g)
