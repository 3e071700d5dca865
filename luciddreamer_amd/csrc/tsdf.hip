// tsdf.hip -- TSDF fusion of depth maps and extraction of a triangle mesh, for gfx950 (include/lucid_raster.h, lr_tsdf_*).
//
// The surface-reconstruction code bases (2DGS, RaDe-GS, PGSR) end by rendering median depth along a trajectory, fusing the maps
// into a truncated signed distance volume and extracting a mesh, with Open3D on the host.  Here both halves run on the device:
//   k_tsdf_integrate : one lattice point per lane, lanes along x.  The point is projected into every frame of the launch with
//                      project_point (float64, the projection of reproject.hip), the voxel's D, W and colour are loaded once,
//                      held in registers across the launch's frames and stored only when a frame touched them.  A gather: no
//                      atomics, one writer per voxel, bit-repeatable.  Cameras travel as kernel arguments,
//                      REPROJECT_FRAMES_PER_LAUNCH frames per launch; later launches follow in stream order.
//   k_tsdf_cells     : one cell per lane: validity, the inside mask of its eight corners, the triangles of its six Kuhn
//                      tetrahedra.  The cell's triangle count goes to a byte, every used edge gets a plain byte store of 1
//                      (many lanes may store to one byte: all store the same value).
//   scans            : k_mask_count / k_mask_rank of mask_scan.h (the scan of rows.hip) over the edge bytes (rank = vertex
//                      index) and over the count bytes (rank = first face of the cell), with k_block_prefix between the two
//                      kernels: one workgroup scans the block sums, which are too many here for each workgroup to sum its own.
//   k_tsdf_vertices  : one edge per lane: the zero crossing and its colour to row rank[edge].
//   k_tsdf_faces     : one cell per lane: its triangles again, as three vertex indices each, from row rank[cell].
// Every float32 operation of the definitions is one IEEE operation in the order the header gives (the file is compiled with
// -ffp-contract=off), so a numpy restatement gives the same bits (tests/tsdf_ref.py).  Winding is combinatorial: it follows from
// the parity of the tetrahedron's axis permutation and the inside mask, never from computed positions.
//
// Traffic: integrate reads 8 (20 with colour) bytes per voxel per launch and writes as many for a touched voxel; the depth
// reads of neighbouring lanes fall on neighbouring pixels.  Extraction is one pass over the corners for the cells, 7 N bytes
// of edge marks, two scans and two emit passes; its workspace is 40 bytes per lattice point (a rank word per edge).
#include "common.h"
#include "lucid_raster.h"
#include "mask_scan.h"            // RS_THREADS, RS_TILE, k_mask_count / k_mask_rank (shared with rows.hip)
#include "project_point.h"        // Cameras, Projected, project_point (shared with reproject.hip and dream.hip)

namespace lr {

namespace {

constexpr int TT = 256;                         // threads per workgroup

struct IntegrateArgs {
    Cameras cam;
    TsdfVolume vol;
    int n_frames, height, width;
    const float* depth;
    const float* color;
    const float* pixel_weight;
    float depth_max, max_weight;
};

// lattice point g -> (i, j, k), x fastest
__device__ __forceinline__ void lattice_ijk(int g, int nx, int ny, int& i, int& j, int& k)
{
    const int nxy = nx * ny;
    k = g / nxy;
    const int r = g - k * nxy;
    j = r / nx;
    i = r - j * nx;
}

__device__ __forceinline__ bool finite_f(float v) { return __builtin_fabsf(v) < __builtin_inff(); }    // false for NaN

__global__ void __launch_bounds__(TT) k_tsdf_integrate(IntegrateArgs a)
{
    const TsdfVolume& vol = a.vol;
    const int N = vol.nx * vol.ny * vol.nz;
    const int g = blockIdx.x * TT + threadIdx.x;
    if (g >= N) return;
    int i, j, k;
    lattice_ijk(g, vol.nx, vol.ny, i, j, k);
    // one multiply, then one add
    const float pt[3] = { (float)i * vol.voxel_size + vol.origin[0], (float)j * vol.voxel_size + vol.origin[1],
                          (float)k * vol.voxel_size + vol.origin[2] };
    float D = vol.tsdf[g], Wt = vol.weight[g];
    float C[3] = { 0.f, 0.f, 0.f };
    const bool with_color = a.color != nullptr;
    if (with_color) {
#pragma unroll
        for (int c = 0; c < 3; c++) C[c] = vol.color[(size_t)g * 3 + c];
    }
    const size_t HW = (size_t)a.height * a.width;
    bool touched = false;
    for (int f = 0; f < a.n_frames; f++) {
        const Projected p = project_point(a.cam, f, pt, 3, 1, 0, a.width, a.height);
        if (!p.valid) continue;
        const size_t pix = (size_t)f * HW + (size_t)p.iv * a.width + p.iu;
        const float d = a.depth[pix];
        if (!(finite_f(d) && d > 0.f && d <= a.depth_max)) continue;
        const float w = a.pixel_weight ? a.pixel_weight[pix] : 1.f;
        if (!(finite_f(w) && w > 0.f)) continue;
        const float sdf = d - p.z;
        if (sdf < -vol.trunc) continue;
        const float q = sdf / vol.trunc;
        const float v = q < 1.f ? q : 1.f;
        const float Wn = Wt + w;
        D = (D * Wt + v * w) / Wn;
        if (with_color) {
#pragma unroll
            for (int c = 0; c < 3; c++) C[c] = (C[c] * Wt + a.color[pix * 3 + c] * w) / Wn;
        }
        Wt = Wn < a.max_weight ? Wn : a.max_weight;
        touched = true;
    }
    if (!touched) return;
    vol.tsdf[g] = D;
    vol.weight[g] = Wt;
    if (with_color) {
#pragma unroll
        for (int c = 0; c < 3; c++) vol.color[(size_t)g * 3 + c] = C[c];
    }
}

// ---- the cell's triangles ----------------------------------------------------------------------------------------------------
// A corner of a cell is a 3-bit code: bit 0 = +x, bit 1 = +y, bit 2 = +z.  Tetrahedron t is the t-th permutation (a, b, c) of
// the axes in lexicographic order: v0 = 0, v1 = e_a, v2 = e_a + e_b, v3 = (1,1,1).  Its orientation det(v1-v0, v2-v0, v3-v0)
// is the permutation's sign.
__device__ __forceinline__ int tet_axis_a(int t) { return t >> 1; }                             // 0 0 1 1 2 2
__device__ __forceinline__ int tet_axis_b(int t) { return ((0x21 >> t) & 1) | (((0x0A >> t) & 1) << 1); }   // 1 2 0 2 0 1
__device__ __forceinline__ bool tet_positive(int t) { return (0x19 >> t) & 1; }                 // + - - + + -

// direction index of the edge between two corners from lower ^ upper, the directions being (1,0,0) (0,1,0) (0,0,1) (1,1,0)
// (1,0,1) (0,1,1) (1,1,1): code 1 -> 0, 2 -> 1, 3 -> 3, 4 -> 2, 5 -> 4, 6 -> 5, 7 -> 6, one nibble each
__device__ __forceinline__ int dir_index(int code)
{
    return (int)((0x65423100u >> (4 * code)) & 7u);
}

// the code of direction d (the inverse of dir_index)
__device__ __forceinline__ int dir_code(int d) { return (int)((0x7653421u >> (4 * d)) & 7u); }

struct CellGeom { int nx, nxy; };

__device__ __forceinline__ int code_offset(int code, const CellGeom& cg)
{
    return (code & 1) + ((code >> 1) & 1) * cg.nx + ((code >> 2) & 1) * cg.nxy;
}

// id of the edge between the tetrahedron's vertices lo < hi (corner codes vc[]) of the cell at lattice point g
__device__ __forceinline__ int edge_id(int g, const int vc[4], int lo, int hi, const CellGeom& cg)
{
    return 7 * (g + code_offset(vc[lo], cg)) + dir_index(vc[lo] ^ vc[hi]);
}

// Calls emit(e0, e1, e2) for every triangle of the cell, in the order of the definition.  cm: bit `code` set = corner inside.
template <class Emit>
__device__ __forceinline__ void cell_triangles(int g, uint32_t cm, const CellGeom& cg, Emit emit)
{
    if (cm == 0u || cm == 0xFFu) return;
    for (int t = 0; t < 6; t++) {
        const int a = tet_axis_a(t), b = tet_axis_b(t);
        const int vc[4] = { 0, 1 << a, (1 << a) | (1 << b), 7 };
        uint32_t m = 0;
#pragma unroll
        for (int v = 0; v < 4; v++) m |= ((cm >> vc[v]) & 1u) << v;
        const int pc = __popc(m);
        if (pc == 0 || pc == 4) continue;
        const bool neg = !tet_positive(t);
        if (pc == 2) {
            // inside p < q, outside r < s: the quad pr, ps, qs, qr.  Its normal at the midpoints is det(q-p, r-p, s-p) times the
            // direction inside -> outside: the tetrahedron's sign times the parity of (p, q, r, s) as a permutation of 0..3.
            const int p = __ffs(m) - 1, q = 31 - __clz(m);
            const uint32_t o = ~m & 15u;
            const int r = __ffs(o) - 1, s = 31 - __clz(o);
            const int inv = (p > r) + (p > s) + (q > r) + (q > s);
            const bool flip = neg != ((inv & 1) != 0);
            const int pr = edge_id(g, vc, p < r ? p : r, p < r ? r : p, cg), ps = edge_id(g, vc, p < s ? p : s, p < s ? s : p, cg);
            const int qs = edge_id(g, vc, q < s ? q : s, q < s ? s : q, cg), qr = edge_id(g, vc, q < r ? q : r, q < r ? r : q, cg);
            if (flip) { emit(pr, qs, ps); emit(pr, qr, qs); }
            else      { emit(pr, ps, qs); emit(pr, qs, qr); }
        } else {
            // one vertex l alone on its side, the others o0 < o1 < o2: the normal of (l o0, l o1, l o2) at the midpoints is
            // det(o0-l, o1-l, o2-l) times the direction away from l: the tetrahedron's sign times (-1)^l.
            const uint32_t lone = pc == 1 ? m : (~m & 15u);
            const int l = __ffs(lone) - 1;
            int o[3], n = 0;
#pragma unroll
            for (int v = 0; v < 4; v++)
                if (v != l) o[n++] = v;
            const bool flip = (neg != ((l & 1) != 0)) != (pc == 3);
            int e[3];
#pragma unroll
            for (int x = 0; x < 3; x++) e[x] = edge_id(g, vc, l < o[x] ? l : o[x], l < o[x] ? o[x] : l, cg);
            if (flip) emit(e[0], e[2], e[1]);
            else      emit(e[0], e[1], e[2]);
        }
    }
}

// the inside mask of the cell at g (bit `code`), and whether all eight corners have weight >= min_weight
__device__ __forceinline__ uint32_t cell_mask(const float* __restrict__ tsdf, const float* __restrict__ weight, int g,
                                              const CellGeom& cg, float min_weight, bool& valid)
{
    uint32_t cm = 0;
    valid = true;
#pragma unroll
    for (int code = 0; code < 8; code++) {
        const int q = g + code_offset(code, cg);
        if (weight) valid = valid && weight[q] >= min_weight;          // NaN is not valid
        cm |= (tsdf[q] < 0.f ? 1u : 0u) << code;
    }
    return cm;
}

__global__ void __launch_bounds__(TT) k_tsdf_cells(TsdfVolume vol, float min_weight, uint8_t* __restrict__ edge_mask,
                                                   uint8_t* __restrict__ cell_count)
{
    const int N = vol.nx * vol.ny * vol.nz;
    const int g = blockIdx.x * TT + threadIdx.x;
    if (g >= N) return;
    int i, j, k;
    lattice_ijk(g, vol.nx, vol.ny, i, j, k);
    int cnt = 0;
    if (i < vol.nx - 1 && j < vol.ny - 1 && k < vol.nz - 1) {
        const CellGeom cg = { vol.nx, vol.nx * vol.ny };
        bool valid;
        const uint32_t cm = cell_mask(vol.tsdf, vol.weight, g, cg, min_weight, valid);
        if (valid)
            cell_triangles(g, cm, cg, [&](int e0, int e1, int e2) {
                edge_mask[e0] = 1;
                edge_mask[e1] = 1;
                edge_mask[e2] = 1;
                cnt++;
            });
    }
    cell_count[g] = (uint8_t)cnt;                   // at most 12
}

__global__ void __launch_bounds__(TT) k_tsdf_vertices(TsdfVolume vol, const uint8_t* __restrict__ edge_mask,
                                                      const uint32_t* __restrict__ edge_rank, long long n_vertices,
                                                      float* __restrict__ out_vertices, float* __restrict__ out_colors)
{
    const int N = vol.nx * vol.ny * vol.nz;
    const int e = blockIdx.x * TT + threadIdx.x;
    if (e >= 7 * N || edge_mask[e] == 0) return;
    const uint32_t row = edge_rank[e];
    if ((long long)row >= n_vertices) return;
    const int p = e / 7, d = e - 7 * p;
    const int code = dir_code(d);
    const CellGeom cg = { vol.nx, vol.nx * vol.ny };
    const int q = p + code_offset(code, cg);
    int i, j, k;
    lattice_ijk(p, vol.nx, vol.ny, i, j, k);
    const int ip[3] = { i, j, k };
    const float Dp = vol.tsdf[p], Dq = vol.tsdf[q];
    const float t = Dp / (Dp - Dq);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float cp = (float)ip[c] * vol.voxel_size + vol.origin[c];
        const float cq = (float)(ip[c] + ((code >> c) & 1)) * vol.voxel_size + vol.origin[c];
        out_vertices[(size_t)row * 3 + c] = cp + t * (cq - cp);
        const float kp = vol.color[(size_t)p * 3 + c], kq = vol.color[(size_t)q * 3 + c];
        out_colors[(size_t)row * 3 + c] = kp + t * (kq - kp);
    }
}

__global__ void __launch_bounds__(TT) k_tsdf_faces(TsdfVolume vol, const uint8_t* __restrict__ cell_count,
                                                   const uint32_t* __restrict__ cell_rank,
                                                   const uint32_t* __restrict__ edge_rank, long long n_faces,
                                                   int* __restrict__ out_faces)
{
    const int N = vol.nx * vol.ny * vol.nz;
    const int g = blockIdx.x * TT + threadIdx.x;
    if (g >= N || cell_count[g] == 0) return;        // a count is only given to a valid cell: its corners are inside the volume
    const CellGeom cg = { vol.nx, vol.nx * vol.ny };
    bool valid;
    const uint32_t cm = cell_mask(vol.tsdf, nullptr, g, cg, 0.f, valid);
    long long row = cell_rank[g];
    cell_triangles(g, cm, cg, [&](int e0, int e1, int e2) {
        if (row < n_faces) {
            out_faces[row * 3 + 0] = (int)edge_rank[e0];
            out_faces[row * 3 + 1] = (int)edge_rank[e1];
            out_faces[row * 3 + 2] = (int)edge_rank[e2];
        }
        row++;
    });
}

struct Layout { size_t counters, edge_mask, cell_count, edge_rank, cell_rank, block_counts, total; };

inline Layout layout(size_t N)
{
    Layout l;
    l.counters = 0;
    l.edge_mask = l.counters + align_up(2 * sizeof(int));
    l.cell_count = l.edge_mask + align_up(7 * N);
    l.edge_rank = l.cell_count + align_up(N);
    l.cell_rank = l.edge_rank + align_up(7 * N * 4);
    l.block_counts = l.cell_rank + align_up(N * 4);
    l.total = l.block_counts + align_up(((7 * N + RS_TILE - 1) / RS_TILE + 1) * 4);   // both scans, one after the other; + the total
    return l;
}

inline unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

size_t tsdf_workspace_bytes(int nx, int ny, int nz) { return layout((size_t)nx * ny * nz).total; }

hipError_t launch_tsdf_integrate(const TsdfIntegrateLaunch& a, hipStream_t s)
{
    const size_t N = (size_t)a.vol.nx * a.vol.ny * a.vol.nz;
    const size_t HW = (size_t)a.height * a.width;
    for (int f0 = 0; f0 < a.n_frames; f0 += REPROJECT_FRAMES_PER_LAUNCH) {
        const int nf = a.n_frames - f0 < REPROJECT_FRAMES_PER_LAUNCH ? a.n_frames - f0 : REPROJECT_FRAMES_PER_LAUNCH;
        IntegrateArgs k;
        for (int c = 0; c < 9; c++) k.cam.K[c] = a.K[c];
        for (int f = 0; f < REPROJECT_FRAMES_PER_LAUNCH; f++) {
            const int g = f < nf ? f0 + f : f0;
            for (int c = 0; c < 9; c++) k.cam.R[f][c] = a.R[(size_t)g * 9 + c];
            for (int c = 0; c < 3; c++) k.cam.T[f][c] = a.T[(size_t)g * 3 + c];
        }
        k.vol = a.vol;
        k.n_frames = nf;
        k.height = a.height;
        k.width = a.width;
        k.depth = a.depth + (size_t)f0 * HW;
        k.color = a.color ? a.color + (size_t)f0 * HW * 3 : nullptr;
        k.pixel_weight = a.pixel_weight ? a.pixel_weight + (size_t)f0 * HW : nullptr;
        k.depth_max = a.depth_max;
        k.max_weight = a.max_weight;
        k_tsdf_integrate<<<blocks_of(N, TT), TT, 0, s>>>(k);
    }
    return hipGetLastError();
}

hipError_t launch_tsdf_extract_count(const TsdfExtractLaunch& a, uint32_t* counts, hipStream_t s)
{
    const size_t N = (size_t)a.vol.nx * a.vol.ny * a.vol.nz;
    const Layout l = layout(N);
    char* ws = static_cast<char*>(a.workspace);
    int* counters = reinterpret_cast<int*>(ws + l.counters);
    uint8_t* edge_mask = reinterpret_cast<uint8_t*>(ws + l.edge_mask);
    uint8_t* cell_count = reinterpret_cast<uint8_t*>(ws + l.cell_count);
    uint32_t* edge_rank = reinterpret_cast<uint32_t*>(ws + l.edge_rank);
    uint32_t* cell_rank = reinterpret_cast<uint32_t*>(ws + l.cell_rank);
    uint32_t* block_counts = reinterpret_cast<uint32_t*>(ws + l.block_counts);
    hipError_t e = hipMemsetAsync(edge_mask, 0, 7 * N, s);
    if (e != hipSuccess) return e;
    k_tsdf_cells<<<blocks_of(N, TT), TT, 0, s>>>(a.vol, a.min_weight, edge_mask, cell_count);
    const int ne = (int)(7 * N), nc = (int)N;
    const unsigned be = blocks_of(7 * N, RS_TILE), bc = blocks_of(N, RS_TILE);
    // the block sums are scanned by one workgroup in between: 7 N / 2048 of them are too many for every workgroup to sum its own
    k_mask_count<false><<<be, RS_THREADS, 0, s>>>(ne, edge_mask, block_counts);
    k_block_prefix<<<1, RS_THREADS, 0, s>>>((int)be, block_counts);
    k_mask_rank<false, true><<<be, RS_THREADS, 0, s>>>(ne, edge_mask, block_counts, edge_rank, counters);
    k_mask_count<true><<<bc, RS_THREADS, 0, s>>>(nc, cell_count, block_counts);
    k_block_prefix<<<1, RS_THREADS, 0, s>>>((int)bc, block_counts);
    k_mask_rank<true, true><<<bc, RS_THREADS, 0, s>>>(nc, cell_count, block_counts, cell_rank, counters + 1);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(counts, counters, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

hipError_t launch_tsdf_extract_emit(const TsdfExtractLaunch& a, hipStream_t s)
{
    const size_t N = (size_t)a.vol.nx * a.vol.ny * a.vol.nz;
    const Layout l = layout(N);
    char* ws = static_cast<char*>(a.workspace);
    const uint8_t* edge_mask = reinterpret_cast<const uint8_t*>(ws + l.edge_mask);
    const uint8_t* cell_count = reinterpret_cast<const uint8_t*>(ws + l.cell_count);
    const uint32_t* edge_rank = reinterpret_cast<const uint32_t*>(ws + l.edge_rank);
    const uint32_t* cell_rank = reinterpret_cast<const uint32_t*>(ws + l.cell_rank);
    if (a.n_vertices > 0)
        k_tsdf_vertices<<<blocks_of(7 * N, TT), TT, 0, s>>>(a.vol, edge_mask, edge_rank, a.n_vertices, a.out_vertices, a.out_colors);
    if (a.n_faces > 0)
        k_tsdf_faces<<<blocks_of(N, TT), TT, 0, s>>>(a.vol, cell_count, cell_rank, edge_rank, a.n_faces, a.out_faces);
    return hipGetLastError();
}

}  // namespace lr
