"""Mesh clean-up on the device (csrc/mesh.hip, lr_mesh_*): connected components, the cluster filter and vertex normals.

The surface-reconstruction code bases (2DGS, RaDe-GS, PGSR) post-process the mesh they fuse with Open3D on the host:
cluster_connected_triangles, keep the largest clusters, remove_unreferenced_vertices, remove_degenerate_triangles,
compute_vertex_normals.  A mesh fused from rendered Gaussian depth carries many small floater components, so the step is part
of the path.  Here it stays on the device, behind tsdf.TSDFVolume.extract_mesh:

    connected_components(faces, n_vertices) -> (face_labels [T], vertex_labels [V], labels [C] ascending, counts [C]), int32
    filter_clusters(vertices, faces, colors=None, normals=None, keep_largest=0, min_faces=1, drop_degenerate=False,
                    return_index=False) -> (vertices', faces'[, colors'][, normals'][, vertex_index, face_index])
    vertex_normals(vertices, faces) -> [V,3] float32
    post_process(vertices, colors, faces, keep_largest=50, min_faces=50, drop_degenerate=True)
        -> (vertices, colors, faces, normals): the filter, then the normals of the cleaned mesh

The definitions (include/lucid_raster.h) are this library's own, stated so that numpy reproduces them to the bit
(tests/mesh_ref.py).  A label is the smallest vertex index of the component (vertex connectivity: two vertices are connected
when a face holds both; Open3D's edge connectivity differs only at a pinch vertex); a face with an index outside [0, V) belongs
to no component and is never kept; a face is kept iff its component has at least max(K-th largest count, min_faces) faces, ties
included; kept rows stay in input order.  Normals are equal-weight sums of unit face normals in int64 fixed point.  Nothing
depends on an arrival order: two runs give the same bits.

Device tensors only: a CPU tensor raises.  float32 vertices and attributes, int32 faces (other dtypes refused); strides and
16-byte alignment are made right by a copy."""
import ctypes

import torch

from . import _lib

SIZE_LIMIT = 2 ** 31 - 2 ** 12        # rows of either array
_INT_MAX = 2 ** 31 - 1


def _dense(t, dtype, cols, dev, what):
    """`dtype` device tensor [n, cols] (or [n] with cols = None), contiguous and 16-byte aligned: the tensor itself or a copy."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"mesh: {what} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"mesh: {what} must be on a HIP device (there is no CPU path)")
    if dev is not None and t.device != dev:
        raise ValueError(f"mesh: {what} is on {t.device}, the mesh on {dev}")
    if t.dtype != dtype:
        raise TypeError(f"mesh: {what} must be {str(dtype).replace('torch.', '')}, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"mesh: {what} must be [n,{cols}], got {tuple(t.shape)}")
    if t.shape[0] > SIZE_LIMIT:
        raise ValueError(f"mesh: {what} has more than 2^31 - 2^12 rows")
    t = t.detach().contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _workspace(V, T, dev):
    n = int(_lib.lib().lr_mesh_workspace_bytes(V, T))
    ws = torch.empty((n,), dtype=torch.uint8, device=dev)
    return ws, n


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _count(value, low, what):
    value = int(value)
    if value < low:
        raise ValueError(f"mesh: {what} must be >= {low}, got {value}")
    return min(value, _INT_MAX)           # beyond any count: the same result


def _components(f, V):
    dev, T = f.device, int(f.shape[0])
    vertex_labels = torch.empty((V,), dtype=torch.int32, device=dev)
    face_labels = torch.empty((T,), dtype=torch.int32, device=dev)
    component_faces = torch.empty((V,), dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace(V, T, dev)
    args = _lib.MeshComponentsArgs(n_vertices=V, n_faces=T, faces=_ptr(f), vertex_labels=_ptr(vertex_labels),
                                   face_labels=_ptr(face_labels), component_faces=_ptr(component_faces), workspace=_ptr(ws),
                                   workspace_bytes=ws_bytes, stream=_stream(dev))
    with _lib.on_device(dev):
        rc = _lib.lib().lr_mesh_components(ctypes.byref(args))
    if rc < 0:
        _lib.raise_for(rc, "mesh.connected_components")
    return face_labels, vertex_labels, component_faces


def connected_components(faces, n_vertices):
    """(face_labels [T], vertex_labels [V], labels [C], counts [C]) int32 on the faces' device.  vertex_labels[v] is the
    smallest vertex index of v's component, face_labels[t] the label of the face's vertices or -1 for a face with an index
    outside [0, n_vertices); labels are, ascending, the labels of the C components that have a face, counts their faces."""
    f = _dense(faces, torch.int32, 3, None, "faces")
    V = int(n_vertices)
    if not 0 <= V <= SIZE_LIMIT:
        raise ValueError(f"mesh: n_vertices must be in [0, 2^31 - 2^12], got {V}")
    face_labels, vertex_labels, component_faces = _components(f, V)
    labels = torch.nonzero(component_faces).reshape(-1).to(torch.int32)          # the list's length is a host value
    return face_labels, vertex_labels, labels, component_faces[labels.long()]


def filter_clusters(vertices, faces, colors=None, normals=None, keep_largest=0, min_faces=1, drop_degenerate=False,
                    return_index=False):
    """Keep the faces of the components that have at least max(c_K, min_faces) faces, c_K being the keep_largest-th largest
    face count (0 with keep_largest = 0 or fewer components: no limit), ties included; with drop_degenerate also drop faces
    with a repeated index or a zero or non-finite area (counts are taken before).  Vertices no kept face uses are removed,
    faces re-indexed, both in input order.  Returns (vertices', faces'), then colors' and normals' where given, then with
    return_index the source rows (vertex_index [V'], face_index [T']) int32.  One host synchronisation (the two sizes)."""
    v = _dense(vertices, torch.float32, 3, None, "vertices")
    dev = v.device
    f = _dense(faces, torch.int32, 3, dev, "faces")
    V, T = int(v.shape[0]), int(f.shape[0])
    attrs = []
    for name, t in (("colors", colors), ("normals", normals)):
        if t is not None:
            t = _dense(t, torch.float32, 3, dev, name)
            if t.shape[0] != V:
                raise ValueError(f"mesh: {name} must be [{V},3], got {tuple(t.shape)}")
        attrs.append(t)
    c, n = attrs
    K, M = _count(keep_largest, 0, "keep_largest"), _count(min_faces, 1, "min_faces")
    L = _lib.lib()
    nv, nf = ctypes.c_longlong(0), ctypes.c_longlong(0)
    ws, ws_bytes = _workspace(V, T, dev)
    args = _lib.MeshFilterArgs(n_vertices=V, n_faces=T, vertices=_ptr(v), faces=_ptr(f), colors=_ptr(c), normals=_ptr(n),
                               keep_largest=K, min_faces=M, drop_degenerate=int(bool(drop_degenerate)), workspace=_ptr(ws),
                               workspace_bytes=ws_bytes, out_n_vertices=ctypes.addressof(nv), out_n_faces=ctypes.addressof(nf),
                               stream=_stream(dev))
    with _lib.on_device(dev):
        rc = L.lr_mesh_filter_count(ctypes.byref(args))
        if rc < 0:
            _lib.raise_for(rc, "mesh.filter_clusters")
        Vo, To = int(nv.value), int(nf.value)
        out_v = torch.empty((Vo, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((To, 3), dtype=torch.int32, device=dev)
        out_c = None if c is None else torch.empty((Vo, 3), dtype=torch.float32, device=dev)
        out_n = None if n is None else torch.empty((Vo, 3), dtype=torch.float32, device=dev)
        vi = torch.empty((Vo,), dtype=torch.int32, device=dev) if return_index else None
        fi = torch.empty((To,), dtype=torch.int32, device=dev) if return_index else None
        args.n_out_vertices, args.n_out_faces = Vo, To
        args.out_vertices, args.out_faces, args.out_colors, args.out_normals = _ptr(out_v), _ptr(out_f), _ptr(out_c), _ptr(out_n)
        args.out_vertex_index, args.out_face_index = _ptr(vi), _ptr(fi)
        rc = L.lr_mesh_filter_emit(ctypes.byref(args))
    if rc < 0:
        _lib.raise_for(rc, "mesh.filter_clusters")
    out = [out_v, out_f] + [t for t in (out_c, out_n) if t is not None]
    if return_index:
        out += [vi, fi]
    return tuple(out)


def vertex_normals(vertices, faces):
    """[V,3] float32: the normalised sum of the unit normals of the faces at each vertex (equal weights, as Open3D's
    compute_vertex_normals), (0,0,0) for a vertex no face with an area uses.  Winding gives the direction."""
    v = _dense(vertices, torch.float32, 3, None, "vertices")
    dev = v.device
    f = _dense(faces, torch.int32, 3, dev, "faces")
    V, T = int(v.shape[0]), int(f.shape[0])
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    ws, ws_bytes = _workspace(V, T, dev)
    args = _lib.MeshNormalsArgs(n_vertices=V, n_faces=T, vertices=_ptr(v), faces=_ptr(f), out_normals=_ptr(out),
                                workspace=_ptr(ws), workspace_bytes=ws_bytes, stream=_stream(dev))
    with _lib.on_device(dev):
        rc = _lib.lib().lr_mesh_vertex_normals(ctypes.byref(args))
    if rc < 0:
        _lib.raise_for(rc, "mesh.vertex_normals")
    return out


def post_process(vertices, colors, faces, keep_largest=50, min_faces=50, drop_degenerate=True):
    """(vertices, colors, faces, normals) of the cleaned mesh: filter_clusters, then vertex_normals of the result.  The
    defaults are 2DGS's post_process_mesh (the 50 largest clusters, none below 50 faces) with degenerate faces removed."""
    v, f, c = filter_clusters(vertices, faces, colors=colors, keep_largest=keep_largest, min_faces=min_faces,
                              drop_degenerate=drop_degenerate)
    return v, c, f, vertex_normals(v, f)
