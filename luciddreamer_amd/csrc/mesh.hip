// mesh.hip -- clean-up of a triangle mesh on the device, for gfx950 (include/lucid_raster.h, lr_mesh_*): connected components,
// the cluster filter and vertex normals.  What 2DGS, RaDe-GS and PGSR do with Open3D on the host after TSDF fusion
// (cluster_connected_triangles, keep the largest clusters, remove_unreferenced_vertices, remove_degenerate_triangles,
// compute_vertex_normals).
//
// Components: a lock-free union-find over parent[V] with min-root hooking.
//   k_mesh_init   : parent[v] = v, component_faces[v] = 0.
//   k_mesh_union  : one face per lane: unite(i0, i1), unite(i0, i2).  parent[x] <= x always, and a word only ever changes from
//                   x (a root) to a smaller index by atomicCAS (the link), and from there to a smaller node of its tree by
//                   atomicMin (path splitting in find_root).  parent is read with agent-scope relaxed atomic loads: a plain
//                   load may be served from this CU's L1 or, for a line another XCD's L2 owns, stay stale for the whole
//                   kernel.  A stale value is still a smaller node of the same tree, so staleness could only cost steps,
//                   never correctness, but it could cost them without bound; the atomic load goes to the coherent level.
//                   Every link is decided by what atomicCAS returns, never by an earlier load.
//   k_mesh_flatten: vertex_labels[v] = root(v).  A root is the smallest index of its tree (every link points down), and after
//                   k_mesh_union every component is one tree: the label is the component's smallest vertex index.
//   k_mesh_count  : face_labels[t] = vertex_labels[i0] (-1 out of range), component_faces[label] += 1 (integer atomicAdd, one
//                   per wave and label).
// The label is canonical and the counts are integers: nothing depends on the order in which lanes arrive.
//
// Filter: k_mesh_roots gathers the non-zero counts (atomicAdd on a cursor: their order varies, the multiset does not),
// k_mesh_threshold (ONE workgroup) selects the K-th largest with a 31-step bitwise select, which reads only that multiset, and
// stores threshold = max(kth, M).  k_mesh_mark writes the face mask and marks the vertices of kept faces with plain byte stores
// of 1 (many lanes may store to one byte: all store the same value).  k_mask_count / k_block_prefix / k_mask_rank of mask_scan.h
// rank both masks; the two totals go to the host (one synchronisation); k_mesh_emit_* write the rows in input order.
//
// Normals: k_mesh_face_normals adds q = rint(n / |n| 2^20) as int64 to the three vertices of every in-range face (integer
// addition is associative: no dependence on the order; the fixed-point idiom of reproject.hip), k_mesh_vertex_normals
// normalises.  Every float64 operation is one IEEE operation in the header's order (the file is compiled with
// -ffp-contract=off), so a numpy restatement gives the same bits (tests/mesh_ref.py).
//
// No kernel dereferences an index outside [0, V).  Row indices are 64-bit: 3 T exceeds an int for T > 2^31 / 3.
// Workspace: 24 bytes per vertex (the int64 sums of the normals; the filter's 21 bytes -- parent, label, count, root list,
// rank, mask -- lie over them) and 9 per face (label, rank, mask).
#include "common.h"
#include "lucid_raster.h"
#include "mask_scan.h"            // RS_THREADS, RS_TILE, k_mask_count / k_block_prefix / k_mask_rank

namespace lr {

namespace {

constexpr int MT = 256;                         // threads per workgroup
constexpr int SEL_THREADS = 1024;               // the one workgroup of k_mesh_threshold
constexpr double NORMAL_SCALE = 1048576.0;      // 2^20

__device__ __forceinline__ long long lane_index() { return (long long)blockIdx.x * MT + threadIdx.x; }

__device__ __forceinline__ int load_parent(const int* parent, int x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x, splitting the path on the way: every node passed is pointed at its grandparent with atomicMin (no return
// value is used: it is not a linking decision).  The grandparent was reached from x through parent words, so it lies in x's
// tree, and trees only ever merge: a word still only decreases, stays <= its index and stays inside its tree, so every walk
// still ends in the tree's one root.  Without it concurrent hooking can leave chains as long as the component (a strip in vertex
// order: parent[k] = k - 1 throughout), and the walks over them are quadratic.
// Ends: parent[x] < x for every x that is not a root, so x strictly decreases and is bounded by 0; no step waits for another lane.
__device__ __forceinline__ int find_root(int* parent, int x)
{
    int p = load_parent(parent, x);
    while (p != x) {
        const int g = load_parent(parent, p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// Joins the trees of a and b.  Ends: every pass either returns or replaces (a, b) by a pair with a smaller sum -- find_root
// never moves up, and after a failed CAS hi becomes the value the CAS returned, which is < hi because hi was no longer a root
// and parent[hi] <= hi.  The sum is bounded by 0.  No pass waits for another lane: a failed CAS is progress made by someone
// else, and its return value is where this lane goes on.
__device__ __forceinline__ void unite(int* parent, int a, int b)
{
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(parent + hi, hi, lo);       // the link exists iff hi was still a root
        if (old == hi) return;
        a = old;                                              // hi's parent since someone else linked it: < hi
        b = lo;
    }
}

__device__ __forceinline__ bool in_range(int i0, int i1, int i2, int V)
{
    return (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
}

__global__ void __launch_bounds__(MT) k_mesh_init(long long V, int* __restrict__ parent, int* __restrict__ component_faces)
{
    const long long v = lane_index();
    if (v >= V) return;
    parent[v] = (int)v;
    component_faces[v] = 0;
}

__global__ void __launch_bounds__(MT) k_mesh_union(long long T, int V, const int* __restrict__ faces, int* parent)
{
    const long long t = lane_index();
    if (t >= T) return;
    const int i0 = faces[t * 3 + 0], i1 = faces[t * 3 + 1], i2 = faces[t * 3 + 2];
    if (!in_range(i0, i1, i2, V)) return;
    unite(parent, i0, i1);
    unite(parent, i0, i2);
}

__global__ void __launch_bounds__(MT) k_mesh_flatten(long long V, int* parent, int* __restrict__ vertex_labels)
{
    const long long v = lane_index();
    if (v >= V) return;
    vertex_labels[v] = find_root(parent, (int)v);
}

// Most faces of a wave share a label (a mesh is mostly its large components), and a million adds to one word queue up at one
// atomic unit: the lanes of a wave that share a label add their number once.  Every lane of the wave runs the loop (todo is
// uniform); integer counts, so the grouping changes no result.
__global__ void __launch_bounds__(MT) k_mesh_count(long long T, int V, const int* __restrict__ faces,
                                                   const int* __restrict__ vertex_labels, int* __restrict__ face_labels,
                                                   int* component_faces)
{
    const long long t = lane_index();
    int label = -1;
    if (t < T) {
        const int i0 = faces[t * 3 + 0], i1 = faces[t * 3 + 1], i2 = faces[t * 3 + 2];
        if (in_range(i0, i1, i2, V)) label = vertex_labels[i0];
        face_labels[t] = label;
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(label >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int l = __shfl(label, leader);
        const unsigned long long same = __ballot(label == l);
        if (lane == leader) atomicAdd(component_faces + l, __popcll(same));
        todo &= ~same;
    }
}

// counters: [0] number of components with a face, [1] threshold, [2] V', [3] T'
__global__ void __launch_bounds__(MT) k_mesh_roots(long long V, const int* __restrict__ component_faces, int* __restrict__ roots,
                                                   int* counters)
{
    const long long v = lane_index();
    if (v >= V) return;
    const int c = component_faces[v];
    if (c > 0) roots[atomicAdd(counters, 1)] = c;
}

// ONE workgroup.  kth = the largest value x with at least K entries >= x (0 when fewer than K entries exist), built from the
// top bit down; threshold = max(kth, M).  K = 0: kth = 0.
__global__ void __launch_bounds__(SEL_THREADS) k_mesh_threshold(int K, int M, const int* __restrict__ roots, int* counters)
{
    __shared__ unsigned s_cnt;
    const int n = counters[0];
    int kth = 0;
    if (K > 0 && n >= K) {                                           // uniform over the workgroup
        for (int bit = 30; bit >= 0; bit--) {
            const int cand = kth | (1 << bit);
            unsigned c = 0;
            for (int i = threadIdx.x; i < n; i += SEL_THREADS) c += roots[i] >= cand ? 1u : 0u;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
            __syncthreads();                                         // the previous step's reads of s_cnt are done
            if (threadIdx.x == 0) s_cnt = 0;
            __syncthreads();
            if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt, c);
            __syncthreads();
            if (s_cnt >= (unsigned)K) kth = cand;
        }
    }
    if (threadIdx.x == 0) counters[1] = kth > M ? kth : M;
}

// The float64 cross product of the header: n = (b - a) x (c - a), L = |n|.
__device__ __forceinline__ double face_cross(const float* __restrict__ vertices, int i0, int i1, int i2, double n[3])
{
    double a[3], e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a[k] = (double)vertices[(size_t)i0 * 3 + k];
        e1[k] = (double)vertices[(size_t)i1 * 3 + k] - a[k];
        e2[k] = (double)vertices[(size_t)i2 * 3 + k] - a[k];
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    return __builtin_sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
}

__device__ __forceinline__ bool positive_finite(double L) { return L > 0.0 && L < __builtin_inf(); }    // false for NaN

__global__ void __launch_bounds__(MT) k_mesh_mark(long long T, int V, const float* __restrict__ vertices,
                                                  const int* __restrict__ faces, const int* __restrict__ face_labels,
                                                  const int* __restrict__ component_faces, const int* __restrict__ counters,
                                                  int drop_degenerate, uint8_t* __restrict__ face_mask, uint8_t* vertex_mask)
{
    const long long t = lane_index();
    if (t >= T) return;
    const int label = face_labels[t];                          // -1: out of range, the indices are not used
    bool keep = label >= 0 && component_faces[label] >= counters[1];
    if (keep) {
        const int i0 = faces[t * 3 + 0], i1 = faces[t * 3 + 1], i2 = faces[t * 3 + 2];
        if (drop_degenerate) {
            if (i0 == i1 || i0 == i2 || i1 == i2) keep = false;
            else {
                double n[3];
                keep = positive_finite(face_cross(vertices, i0, i1, i2, n));
            }
        }
        if (keep) {
            vertex_mask[i0] = 1;
            vertex_mask[i1] = 1;
            vertex_mask[i2] = 1;
        }
    }
    face_mask[t] = keep ? 1 : 0;
}

__global__ void __launch_bounds__(MT) k_mesh_emit_vertices(long long V, const uint8_t* __restrict__ vertex_mask,
                                                           const uint32_t* __restrict__ vertex_rank, long long n_out,
                                                           const float* __restrict__ vertices, const float* __restrict__ colors,
                                                           const float* __restrict__ normals, float* __restrict__ out_vertices,
                                                           float* __restrict__ out_colors, float* __restrict__ out_normals,
                                                           int* __restrict__ out_index)
{
    const long long v = lane_index();
    if (v >= V || vertex_mask[v] == 0) return;
    const long long row = vertex_rank[v];
    if (row >= n_out) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        out_vertices[row * 3 + k] = vertices[v * 3 + k];
        if (colors) out_colors[row * 3 + k] = colors[v * 3 + k];
        if (normals) out_normals[row * 3 + k] = normals[v * 3 + k];
    }
    if (out_index) out_index[row] = (int)v;
}

__global__ void __launch_bounds__(MT) k_mesh_emit_faces(long long T, const uint8_t* __restrict__ face_mask,
                                                        const uint32_t* __restrict__ face_rank, long long n_out,
                                                        const int* __restrict__ faces, const uint32_t* __restrict__ vertex_rank,
                                                        int* __restrict__ out_faces, int* __restrict__ out_index)
{
    const long long t = lane_index();
    if (t >= T || face_mask[t] == 0) return;                   // a kept face is in range
    const long long row = face_rank[t];
    if (row >= n_out) return;
#pragma unroll
    for (int k = 0; k < 3; k++) out_faces[row * 3 + k] = (int)vertex_rank[faces[t * 3 + k]];
    if (out_index) out_index[row] = (int)t;
}

__global__ void __launch_bounds__(MT) k_mesh_face_normals(long long T, int V, const float* __restrict__ vertices,
                                                          const int* __restrict__ faces, unsigned long long* sums)
{
    const long long t = lane_index();
    if (t >= T) return;
    const int idx[3] = { faces[t * 3 + 0], faces[t * 3 + 1], faces[t * 3 + 2] };
    if (!in_range(idx[0], idx[1], idx[2], V)) return;
    double n[3];
    const double L = face_cross(vertices, idx[0], idx[1], idx[2], n);
    if (!positive_finite(L)) return;
    unsigned long long q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = (unsigned long long)(long long)rint(n[k] / L * NORMAL_SCALE);     // two's complement sums
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) atomicAdd(sums + (size_t)idx[c] * 3 + k, q[k]);
}

__global__ void __launch_bounds__(MT) k_mesh_vertex_normals(long long V, const unsigned long long* __restrict__ sums,
                                                            float* __restrict__ out_normals)
{
    const long long v = lane_index();
    if (v >= V) return;
    double s[3];
#pragma unroll
    for (int k = 0; k < 3; k++) s[k] = (double)(long long)sums[v * 3 + k];
    const double S = __builtin_sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) out_normals[v * 3 + k] = S == 0.0 ? 0.f : (float)(s[k] / S);
}

// The filter's arrays lie over the normals' sums: the two never run on one workspace at the same time.
struct Layout {
    size_t counters, parent, vertex_labels, component_faces, roots, vertex_rank, vertex_mask, face_labels, face_rank, face_mask,
        block_counts, total;
    size_t sums;
};

inline Layout layout(size_t V, size_t T)
{
    Layout l;
    l.counters = 0;
    size_t o = align_up(4 * sizeof(int));
    l.sums = o;
    l.parent = o;          o += align_up(V * 4);
    l.vertex_labels = o;   o += align_up(V * 4);
    l.component_faces = o; o += align_up(V * 4);
    l.roots = o;           o += align_up(V * 4);
    l.vertex_rank = o;     o += align_up(V * 4);
    l.vertex_mask = o;     o += align_up(V);
    const size_t sums_end = l.sums + align_up(V * 24);
    if (o < sums_end) o = sums_end;
    l.face_labels = o;     o += align_up(T * 4);
    l.face_rank = o;       o += align_up(T * 4);
    l.face_mask = o;       o += align_up(T);
    l.block_counts = o;    o += align_up(((V > T ? V : T) / RS_TILE + 2) * 4);      // one scan after the other; + the total
    l.total = o;
    return l;
}

inline unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// parent and component_faces of the whole mesh; labels of its vertices and faces
hipError_t components(long long V, long long T, const int* faces, int* parent, int* vertex_labels, int* face_labels,
                      int* component_faces, hipStream_t s)
{
    if (V > 0) k_mesh_init<<<blocks_of(V, MT), MT, 0, s>>>(V, parent, component_faces);
    if (V > 0 && T > 0) k_mesh_union<<<blocks_of(T, MT), MT, 0, s>>>(T, (int)V, faces, parent);
    if (V > 0) k_mesh_flatten<<<blocks_of(V, MT), MT, 0, s>>>(V, parent, vertex_labels);
    if (T > 0) k_mesh_count<<<blocks_of(T, MT), MT, 0, s>>>(T, (int)V, faces, vertex_labels, face_labels, component_faces);
    return hipGetLastError();
}

}  // namespace

size_t mesh_workspace_bytes(long long n_vertices, long long n_faces) { return layout((size_t)n_vertices, (size_t)n_faces).total; }

hipError_t launch_mesh_components(const MeshComponentsLaunch& a, hipStream_t s)
{
    const Layout l = layout((size_t)a.n_vertices, (size_t)a.n_faces);
    int* parent = reinterpret_cast<int*>(static_cast<char*>(a.workspace) + l.parent);
    return components(a.n_vertices, a.n_faces, a.faces, parent, a.vertex_labels, a.face_labels, a.component_faces, s);
}

hipError_t launch_mesh_filter_count(const MeshFilterLaunch& a, uint32_t* counts, hipStream_t s)
{
    const long long V = a.n_vertices, T = a.n_faces;
    const Layout l = layout((size_t)V, (size_t)T);
    char* ws = static_cast<char*>(a.workspace);
    int* counters = reinterpret_cast<int*>(ws + l.counters);
    int* parent = reinterpret_cast<int*>(ws + l.parent);
    int* vertex_labels = reinterpret_cast<int*>(ws + l.vertex_labels);
    int* component_faces = reinterpret_cast<int*>(ws + l.component_faces);
    int* roots = reinterpret_cast<int*>(ws + l.roots);
    uint32_t* vertex_rank = reinterpret_cast<uint32_t*>(ws + l.vertex_rank);
    uint8_t* vertex_mask = reinterpret_cast<uint8_t*>(ws + l.vertex_mask);
    int* face_labels = reinterpret_cast<int*>(ws + l.face_labels);
    uint32_t* face_rank = reinterpret_cast<uint32_t*>(ws + l.face_rank);
    uint8_t* face_mask = reinterpret_cast<uint8_t*>(ws + l.face_mask);
    uint32_t* block_counts = reinterpret_cast<uint32_t*>(ws + l.block_counts);
    hipError_t e = hipMemsetAsync(counters, 0, 4 * sizeof(int), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(vertex_mask, 0, (size_t)V, s);
    if (e != hipSuccess) return e;
    e = components(V, T, a.faces, parent, vertex_labels, face_labels, component_faces, s);
    if (e != hipSuccess) return e;
    k_mesh_roots<<<blocks_of(V, MT), MT, 0, s>>>(V, component_faces, roots, counters);
    k_mesh_threshold<<<1, SEL_THREADS, 0, s>>>(a.keep_largest, a.min_faces, roots, counters);
    k_mesh_mark<<<blocks_of(T, MT), MT, 0, s>>>(T, (int)V, a.vertices, a.faces, face_labels, component_faces, counters,
                                                a.drop_degenerate, face_mask, vertex_mask);
    const unsigned bv = blocks_of(V, RS_TILE), bf = blocks_of(T, RS_TILE);
    k_mask_count<false><<<bv, RS_THREADS, 0, s>>>((int)V, vertex_mask, block_counts);
    k_block_prefix<<<1, RS_THREADS, 0, s>>>((int)bv, block_counts);
    k_mask_rank<false, true><<<bv, RS_THREADS, 0, s>>>((int)V, vertex_mask, block_counts, vertex_rank, counters + 2);
    k_mask_count<false><<<bf, RS_THREADS, 0, s>>>((int)T, face_mask, block_counts);
    k_block_prefix<<<1, RS_THREADS, 0, s>>>((int)bf, block_counts);
    k_mask_rank<false, true><<<bf, RS_THREADS, 0, s>>>((int)T, face_mask, block_counts, face_rank, counters + 3);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(counts, counters + 2, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

hipError_t launch_mesh_filter_emit(const MeshFilterLaunch& a, hipStream_t s)
{
    const long long V = a.n_vertices, T = a.n_faces;
    const Layout l = layout((size_t)V, (size_t)T);
    char* ws = static_cast<char*>(a.workspace);
    const uint32_t* vertex_rank = reinterpret_cast<const uint32_t*>(ws + l.vertex_rank);
    const uint8_t* vertex_mask = reinterpret_cast<const uint8_t*>(ws + l.vertex_mask);
    const uint32_t* face_rank = reinterpret_cast<const uint32_t*>(ws + l.face_rank);
    const uint8_t* face_mask = reinterpret_cast<const uint8_t*>(ws + l.face_mask);
    if (a.n_out_vertices > 0)
        k_mesh_emit_vertices<<<blocks_of(V, MT), MT, 0, s>>>(V, vertex_mask, vertex_rank, a.n_out_vertices, a.vertices, a.colors,
                                                             a.normals, a.out_vertices, a.out_colors, a.out_normals,
                                                             a.out_vertex_index);
    if (a.n_out_faces > 0)
        k_mesh_emit_faces<<<blocks_of(T, MT), MT, 0, s>>>(T, face_mask, face_rank, a.n_out_faces, a.faces, vertex_rank,
                                                          a.out_faces, a.out_face_index);
    return hipGetLastError();
}

hipError_t launch_mesh_vertex_normals(const MeshNormalsLaunch& a, hipStream_t s)
{
    const long long V = a.n_vertices, T = a.n_faces;
    const Layout l = layout((size_t)V, (size_t)T);
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(static_cast<char*>(a.workspace) + l.sums);
    if (T == 0) return hipMemsetAsync(a.out_normals, 0, (size_t)V * 3 * sizeof(float), s);
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)V * 24, s);
    if (e != hipSuccess) return e;
    k_mesh_face_normals<<<blocks_of(T, MT), MT, 0, s>>>(T, (int)V, a.vertices, a.faces, sums);
    k_mesh_vertex_normals<<<blocks_of(V, MT), MT, 0, s>>>(V, sums, a.out_normals);
    return hipGetLastError();
}

}  // namespace lr
