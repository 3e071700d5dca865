// render_normals.hip -- the rendered normal map of a finished forward (the per-pixel blend of the Gaussians' normals that 2DGS,
// RaDe-GS and PGSR compare with the normals of the rendered depth) and its gradient, for gfx950.
//
// Per-Gaussian normal (scales + rotations only; cov3D_precomp has none).  k = argmin of the three scales as given (activated, or
// in raw mode the stored log-scales: an exact comparison of inputs, lowest index on ties, so an isotropic Gaussian takes axis 0);
// n_world = R(q)[:, k], R the quaternion matrix with Sigma = R S^2 R^T (activated mode: q as given, raw mode: q / max(|q|, eps) by
// act_quat_inv_norm); n_view = W n_world, W the rotation part of the view matrix (x right, y down, z forward: the axes of
// normals.depth_normals); turned towards the camera once per Gaussian: n_view . p_view > 0 -> n_view = -n_view, p_view the
// view-space mean.  The axis and the sign are constants of the view, as the sort order is.
//     gauss_normals [P,4] float32 : {n_view.xyz, sign (k + 1)}, zeros for radii <= 0
//
// Per-pixel map.  The walk of k_render_distort (tile_walk.h: the forward's skips, 0.99 clamp and 1e-4 stop, bit for bit its T
// sequence), w_i = alpha_i T_i:
//     normals [3,H,W] float32 : N = sum_i w_i n_i; no background term, no normalisation (|N| <= alpha); exact zeros for a pixel
//                               with no layer, for P = 0 and for an overflowed async view
//
// Gradient, g = dL/dN of the pixel, c_i = n_i . g:
//     dL/dn_i += w_i g          dL/dalpha_i = T_i c_i - S_i / (1 - alpha_i),   S_i = sum_{k>i} w_k c_k = N.g - sum_{k<=i} w_k c_k
// S_i is taken FRONT TO BACK on the forward's own T sequence, as k_distort_bwd takes its S_i.  The clamp is not differentiated; the
// skips, the stop and the order are constants.  alpha = opacity G reaches mean2D, conic and opacity with the expressions of the
// blend backward's flush (render_bwd.hip); dL/dn_i goes to the slot's three colour floats, which the per-Gaussian backward
// (k_gauss_bwd, as it stands) sums per Gaussian into the row it is given as dL_dcolor: dL_dgauss_normal [P,3].
//
// k_normals_bwd: the shape of k_distort_bwd, with NINE sums per list entry (D dx, D dy, D dx^2, D dx dy, D dy^2, D with
// D = opacity G dL/dalpha, and the three components of sum w g): eight through reduce8 and two row sums, the ninth through a row
// sum of its own whose four row partials take a column each -- 12 columns x 4 waves x 128 entries = 24 KB of per-wave accumulators
// plus 6.5 KB of staging, five workgroups per CU by LDS.  The flush writes ONE plain 48-byte GradRec per instance --
// {mean2D x, y, conic a, b | conic c, opacity, dn.x, dn.y | dn.z, 0, 0, 0} -- exact zeros for an entry no pixel blended, every slot
// of every list position written.  No global float atomics: bit-repeatable.  It OVERWRITES inst_grad (lr_distortion_backward's
// ordering rule).
// k_normal_rot_bwd: dL_dgauss_normal -> un-flip -> W^T -> the Jacobian of column k of R(q) -> (raw: (g - q (q.g)) / |r|), ADDED
// into dL_drot.  Nothing flows to scales or the mean through the axis choice or the sign.
#include "common.h"
#include "gauss_project.h"
#include "tile_walk.h"
#include "wave_reduce.h"

namespace lr {

namespace {

constexpr int RN_BATCH = 256;           // forward: staged list entries per round (10 KB + 2 KB of LDS)
constexpr int RNB_BATCH = 128;          // backward: staged list entries per round
constexpr int RNB_COLS = 12;            // sums per entry and wave: reduce8's eight, then the four row partials of the ninth

// ---- per-Gaussian normal ------------------------------------------------------------------------------------------------------
// column k of R(q) = row k of quat_rotation's M3 read across (c[col][row], c[j] = row j of R)
__device__ __forceinline__ V3 quat_column(float r, float x, float y, float z, int k)
{
    const M3 Rm = quat_rotation(r, x, y, z);
    if (k == 0) return { Rm.c[0][0], Rm.c[1][0], Rm.c[2][0] };       // (no dynamic index: the matrix stays in registers)
    if (k == 1) return { Rm.c[0][1], Rm.c[1][1], Rm.c[2][1] };
    return { Rm.c[0][2], Rm.c[1][2], Rm.c[2][2] };
}

template <bool RAW>
__global__ void __launch_bounds__(256)
k_gauss_normals(int P, const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
                const float* __restrict__ V, const int* __restrict__ radii, float4* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    if (radii[i] <= 0) { out[i] = make_float4(0.f, 0.f, 0.f, 0.f); return; }
    const float s0 = scales[3 * (size_t)i], s1 = scales[3 * (size_t)i + 1], s2 = scales[3 * (size_t)i + 2];
    int k = 0;
    float sm = s0;
    if (s1 < sm) { k = 1; sm = s1; }
    if (s2 < sm) { k = 2; }
    float4 q = reinterpret_cast<const float4*>(rotations)[i];
    if (RAW) {
        const float inv = act_quat_inv_norm(q.x, q.y, q.z, q.w);
        q.x *= inv; q.y *= inv; q.z *= inv; q.w *= inv;
    }
    const V3 nw = quat_column(q.x, q.y, q.z, q.w, k);
    const float mx = means3D[3 * (size_t)i], my = means3D[3 * (size_t)i + 1], mz = means3D[3 * (size_t)i + 2];
    float nx = V[0] * nw.x + V[4] * nw.y + V[8] * nw.z;
    float ny = V[1] * nw.x + V[5] * nw.y + V[9] * nw.z;
    float nz = V[2] * nw.x + V[6] * nw.y + V[10] * nw.z;
    const float vx = V[0] * mx + V[4] * my + V[8] * mz + V[12];
    const float vy = V[1] * mx + V[5] * my + V[9] * mz + V[13];
    const float vz = V[2] * mx + V[6] * my + V[10] * mz + V[14];
    float sign = 1.0f;
    if (nx * vx + ny * vy + nz * vz > 0.0f) { nx = -nx; ny = -ny; nz = -nz; sign = -1.0f; }
    out[i] = make_float4(nx, ny, nz, sign * (float)(k + 1));
}

// dL_dgauss_normal -> dL_drot (added); one thread per Gaussian with radii > 0
template <bool RAW>
__global__ void __launch_bounds__(256)
k_normal_rot_bwd(int P, const float* __restrict__ rotations, const float* __restrict__ V, const int* __restrict__ radii,
                 const GeomHeader* __restrict__ hdr, const float4* __restrict__ gauss_normals,
                 const float* __restrict__ dL_dgauss_normal, float4* __restrict__ dL_drot)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    if (hdr->overflow != 0u) return;                                  // async mode: an overflowed view contributes nothing
    if (radii[i] <= 0) return;
    const float tag = gauss_normals[i].w;
    if (tag == 0.0f) return;
    const float sign = tag < 0.0f ? -1.0f : 1.0f;
    const int k = (int)fabsf(tag) - 1;
    const float dx = sign * dL_dgauss_normal[3 * (size_t)i], dy = sign * dL_dgauss_normal[3 * (size_t)i + 1],
                dz = sign * dL_dgauss_normal[3 * (size_t)i + 2];
    // W^T
    const float a = V[0] * dx + V[1] * dy + V[2] * dz;
    const float b = V[4] * dx + V[5] * dy + V[6] * dz;
    const float c = V[8] * dx + V[9] * dy + V[10] * dz;
    float4 q = reinterpret_cast<const float4*>(rotations)[i];
    float inv = 1.0f;
    if (RAW) {
        inv = act_quat_inv_norm(q.x, q.y, q.z, q.w);
        q.x *= inv; q.y *= inv; q.z *= inv; q.w *= inv;
    }
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    float gr, gx, gy, gz;
    if (k == 0) {            // (1 - 2 (yy + zz), 2 (xy + rz), 2 (xz - ry))
        gr = 2.f * (z * b - y * c);
        gx = 2.f * (y * b + z * c);
        gy = -4.f * y * a + 2.f * (x * b - r * c);
        gz = -4.f * z * a + 2.f * (r * b + x * c);
    } else if (k == 1) {     // (2 (xy - rz), 1 - 2 (xx + zz), 2 (yz + rx))
        gr = 2.f * (x * c - z * a);
        gx = -4.f * x * b + 2.f * (y * a + r * c);
        gy = 2.f * (x * a + z * c);
        gz = -4.f * z * b + 2.f * (y * c - r * a);
    } else {                 // (2 (xz + ry), 2 (yz - rx), 1 - 2 (xx + yy))
        gr = 2.f * (y * a - x * b);
        gx = -4.f * x * c + 2.f * (z * a - r * b);
        gy = -4.f * y * c + 2.f * (r * a + z * b);
        gz = 2.f * (x * a + y * b);
    }
    if (RAW) {               // through q = r / |r|: (g - q (q.g)) / |r|, as gauss_backward_one
        const float qg = r * gr + x * gx + y * gy + z * gz;
        gr = (gr - r * qg) * inv; gx = (gx - x * qg) * inv; gy = (gy - y * qg) * inv; gz = (gz - z * qg) * inv;
    }
    float4 o = dL_drot[i];
    o.x += gr; o.y += gx; o.z += gy; o.w += gz;
    dL_drot[i] = o;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <bool STRICT>
__global__ void __launch_bounds__(WALK_THREADS)
k_render_normals(int W, int H, int gx, int num_tiles, int tile_map, const uint2* __restrict__ ranges,
                 const char* __restrict__ bin_base, const GaussRec* __restrict__ rec, const GeomHeader* __restrict__ hdr,
                 const float4* __restrict__ gauss_normals, float* __restrict__ out)
{
    __shared__ float4 s_q0[RN_BATCH];       // WalkPlanes; the value kept in s_q1[].z: n.z
    __shared__ float4 s_q1[RN_BATCH];
    __shared__ float2 s_q3[RN_BATCH];
    __shared__ float2 s_n[RN_BATCH];        // n.x, n.y of each staged entry
    __shared__ int s_wdone[WALK_WAVES];

    const int tile = blend_tile(tile_map, num_tiles);
    if (tile < 0) return;
    const QuadLane q = quad_lane(tile, gx, W, H);
    const TileList tl = tile_list(hdr, ranges, bin_base, tile);     // overflowed: empty, zeros everywhere

    float T = 1.0f, Nx = 0.0f, Ny = 0.0f, Nz = 0.0f;
    uint64_t done = __builtin_amdgcn_ballot_w64(!q.inside);           // pixels that have stopped (or lie outside the image)

    tile_walk<STRICT, RN_BATCH>(
        q, tl, rec, WalkPlanes{s_q0, s_q1, s_q3, s_wdone}, done,
        [&](int slot, uint32_t id, float) {
            const float4 n = gauss_normals[id];
            s_n[slot] = make_float2(n.x, n.y);
            return n.z;
        },
        [&](int j, float nz, float alpha, uint64_t use) {
            const float test_T = T * (1.0f - alpha);
            const uint64_t stop = use & __builtin_amdgcn_ballot_w64(test_T < 0.0001f);
            if (__builtin_amdgcn_inverse_ballot_w64(use & ~stop)) {
                const float wt = alpha * T;
                const float2 n = s_n[j];
                Nx = __builtin_fmaf(wt, n.x, Nx);
                Ny = __builtin_fmaf(wt, n.y, Ny);
                Nz = __builtin_fmaf(wt, nz, Nz);
                T = test_T;
            }
            return stop;
        },
        [](int, float, uint64_t) {});

    if (q.inside) {
        const size_t hw = (size_t)W * H, pix = (size_t)q.py * W + q.px;
        out[pix] = Nx;
        out[hw + pix] = Ny;
        out[2 * hw + pix] = Nz;
    }
}

// a view without a list to read (P = 0): zeros everywhere
__global__ void __launch_bounds__(256) k_normals_fill(long long n, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 0.0f;
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rn_zero_slot(float4* __restrict__ inst_grad, uint32_t e)
{
    float4* slot = inst_grad + 3 * (size_t)e;
    slot[0] = make_float4(0.f, 0.f, 0.f, 0.f); slot[1] = slot[0]; slot[2] = slot[0];
}

// Launch bounds: at most 128 VGPRs, so that with 31 KB of LDS five workgroups fit a CU
template <bool STRICT>
__global__ void __launch_bounds__(WALK_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_normals_bwd(int W, int H, int gx, int num_tiles, int tile_map, const uint2* __restrict__ ranges, char* __restrict__ bin_base,
              const GaussRec* __restrict__ rec, const GeomHeader* __restrict__ hdr, const float* __restrict__ dL_dnormals,
              const float* __restrict__ normals, const float4* __restrict__ gauss_normals)
{
    __shared__ float4 s_q0[RNB_BATCH];      // x, y, Ap, Bp (x log2 e; strict: conic a, b)
    __shared__ float4 s_q1[RNB_BATCH];      // Cp (strict: conic c), opacity, n.z, qmax
    __shared__ float4 s_q2[RNB_BATCH];      // -b/c, -b/a, n.x, n.y
    __shared__ uint32_t s_id[RNB_BATCH];    // emission index (instance slot) of each staged entry
    __shared__ __attribute__((aligned(16))) float s_acc[RNB_BATCH][WALK_WAVES][RNB_COLS];   // every wave its own copy: plain stores, summed in wave order
    __shared__ int s_wdone[WALK_WAVES];

    const int tile = blend_tile(tile_map, num_tiles);
    if (tile < 0) return;
    if (hdr->overflow != 0u) return;                                 // async mode: an overflowed view contributes nothing
    const uint2 range = ranges[tile];
    const int total = (int)(range.y - range.x);
    if (total == 0) return;
    const QuadLane q = quad_lane(tile, gx, W, H);
    const int tid = q.tid, w = q.w, l = q.l, px = q.px, py = q.py;
    const bool inside = q.inside;
    const float pxf = q.pxf, pyf = q.pyf, bx0 = q.bx0, bx1 = q.bx1, by0 = q.by0, by1 = q.by1;

    const BinLayout BL = bin_layout((long long)hdr->bin_bound);
    const uint32_t* __restrict__ point_list = reinterpret_cast<const uint32_t*>(bin_base + BL.point_list) + range.x;
    const uint32_t* __restrict__ list_gid = reinterpret_cast<const uint32_t*>(bin_base + BL.list_gid) + range.x;
    float4* __restrict__ inst_grad = reinterpret_cast<float4*>(bin_base + BL.inst_grad);

    // the pixel: upstream and N.g; a pixel without an upstream adds exact zeros and is done from the start
    float gX = 0.0f, gY = 0.0f, gZ = 0.0f, Ng = 0.0f;
    if (inside) {
        const size_t hw = (size_t)W * H, pix = (size_t)py * W + px;
        gX = dL_dnormals[pix]; gY = dL_dnormals[hw + pix]; gZ = dL_dnormals[2 * hw + pix];
        Ng = __builtin_fmaf(normals[2 * hw + pix], gZ, __builtin_fmaf(normals[hw + pix], gY, normals[pix] * gX));
    }
    float T = 1.0f, C = 0.0f;                                         // C = sum_{k<=i} w_k c_k
    uint64_t done = __builtin_amdgcn_ballot_w64(!inside || (gX == 0.0f && gY == 0.0f && gZ == 0.0f));
    bool wave_done = done == ~0ull;
    const float ddelx_dx = (float)(0.5 * W), ddely_dy = (float)(0.5 * H);    // the NDC scale of dL/dmean2D (render_bwd.hip)

    const int row = l >> 4;
    const int col_a = (row == 0) ? 0 : (row == 1) ? 2 : (row == 2) ? 1 : 3;  // reduce8: rows hold terms {0, 2, 1, 3}
    const bool row_leader = (l & 15) == 0;

    for (int base = 0; base < total; base += RNB_BATCH) {
        if (l == 0) s_wdone[w] = wave_done ? 1 : 0;
        lds_barrier();                                                // (previous round fully flushed)
        if (s_wdone[0] + s_wdone[1] + s_wdone[2] + s_wdone[3] == WALK_WAVES) {
            // every pixel of the tile has stopped: the rest of the list was blended by nobody, its slots read as zero
            for (int p = base + tid; p < total; p += WALK_THREADS) rn_zero_slot(inst_grad, point_list[p]);
            break;
        }
        const int cnt = min(RNB_BATCH, total - base);
        if (tid < cnt) {
            const uint32_t id = list_gid[base + tid];
            const float4* gr = reinterpret_cast<const float4*>(rec + id);
            const float4 a = gr[0], b = gr[1], c = gr[2];
            const float4 n = gauss_normals[id];
            s_q0[tid] = STRICT ? make_float4(a.x, a.y, a.z, a.w) : make_float4(a.x, a.y, (-0.5f * LOG2E) * a.z, -LOG2E * a.w);
            s_q1[tid] = STRICT ? make_float4(b.x, b.y, n.z, c.z) : make_float4((-0.5f * LOG2E) * b.x, b.y, n.z, LOG2E * c.z);
            s_q2[tid] = make_float4(-a.w / b.x, -a.w / a.z, n.x, n.y);
            s_id[tid] = point_list[base + tid];
        }
        {
            float4* z4 = reinterpret_cast<float4*>(&s_acc[0][0][0]);
            const int n4 = cnt * (WALK_WAVES * RNB_COLS / 4);
            for (int i = tid; i < n4; i += WALK_THREADS) z4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        lds_barrier();

        if (!wave_done) {
            for (int sb = 0; sb < cnt; sb += 64) {
                bool hit = false;
                const int jl = sb + l;
                if (jl < cnt) {
                    const float4 a = s_q0[jl];
                    const float4 b = s_q1[jl];
                    const float4 r = s_q2[jl];
                    const float ca = STRICT ? a.z : -2.0f * a.z, cb = STRICT ? a.w : -a.w, cc = STRICT ? b.x : -2.0f * b.x;
                    hit = box_hit(a.x, a.y, ca, cb, cc, r.x, r.y, b.w, bx0, bx1, by0, by1);
                }
                uint64_t mask = __ballot(hit);
                while (mask) {
                    const int k = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const int j = sb + k;
                    const float4 a = s_q0[j];
                    const float4 b = s_q1[j];
                    const float dx = a.x - pxf, dy = a.y - pyf;
                    float r0, r1, power;
                    gauss_row<STRICT>(a.w, b.x, dy, r0, r1);
                    const float t = b.y * gauss_weight<STRICT>(a.z, a.w, b.x, r0, r1, dx, power);   // alpha before the 0.99 clamp
                    const float alpha_f = fminf(0.99f, t);
                    const float test_T = T * (1.0f - alpha_f);
                    // the forward's decisions, on the forward's values
                    const uint64_t use = ~done & __builtin_amdgcn_ballot_w64(power <= 0.0f) & __builtin_amdgcn_ballot_w64(alpha_f >= 1.0f / 255.0f);
                    const uint64_t stop = use & __builtin_amdgcn_ballot_w64(test_T < 0.0001f);
                    const uint64_t blend = use & ~stop;
                    done |= stop;
                    if (blend != 0ull) {
                        // a pixel that does not blend the entry takes it as a layer with alpha = 0: every term is an exact zero
                        const bool bl = __builtin_amdgcn_inverse_ballot_w64(blend);
                        const float4 nn = s_q2[j];
                        const float tm = bl ? t : 0.0f;
                        const float alpha = fminf(0.99f, tm);
                        const float wt = alpha * T;
                        const float c = __builtin_fmaf(b.z, gZ, __builtin_fmaf(nn.w, gY, nn.z * gX));   // n . g
                        C = __builtin_fmaf(wt, c, C);
                        const float rinv = __builtin_amdgcn_rcpf(1.0f - alpha);
                        const float dNda = __builtin_fmaf(T, c, -((Ng - C) * rinv));
                        const float dop = tm * dNda;                                        // opacity x G x dL/dalpha
                        T = bl ? test_T : T;
                        const float mx = dop * dx, my = dop * dy;
                        float ra = mx, rb = my * dy;
                        reduce8(ra, my, mx * dx, mx * dy, rb, dop, wt * gX, wt * gY);
                        ra = row_sum(ra);
                        rb = row_sum(rb);
                        const float rc = row_sum(wt * gZ);                                  // the ninth: four row partials
                        if (row_leader) {
                            float* dst = &s_acc[j][w][0];
                            dst[col_a] = ra;
                            dst[4 + col_a] = rb;
                            dst[8 + row] = rc;
                        }
                    }
                    if (done == ~0ull) break;
                }
                if (done == ~0ull) { wave_done = true; break; }
            }
        }
        lds_barrier();
        if (tid < cnt) {
            float a12[RNB_COLS];
#pragma unroll
            for (int k = 0; k < RNB_COLS; k++) {
                float v = s_acc[tid][0][k];
#pragma unroll
                for (int a = 1; a < WALK_WAVES; a++) v += s_acc[tid][a][k];                  // fixed order over the waves
                a12[k] = v;
            }
            const float dnz = (a12[8] + a12[9]) + (a12[10] + a12[11]);
            // the factors that are constant per Gaussian, as the blend backward's flush applies them
            const float4 q0 = s_q0[tid], q1 = s_q1[tid];
            const float ca = STRICT ? q0.z : (-2.0f * LN2) * q0.z, cb = STRICT ? q0.w : -LN2 * q0.w,
                        cc = STRICT ? q1.x : (-2.0f * LN2) * q1.x, o = q1.y;
            const float sx = a12[0], sy = a12[1], h = -0.5f;
            const float dopac = o > 0.f ? a12[5] * __builtin_amdgcn_rcpf(o) : 0.f;
            float4* slot = inst_grad + 3 * (size_t)s_id[tid];
            slot[0] = make_float4((-ca * sx - cb * sy) * ddelx_dx, (-cc * sy - cb * sx) * ddely_dy, h * a12[2], h * a12[3]);
            slot[1] = make_float4(h * a12[4], dopac, a12[6], a12[7]);
            slot[2] = make_float4(dnz, 0.f, 0.f, 0.f);
        }
    }
}

}  // namespace

void launch_gauss_normals(int P, bool raw, const float* means3D, const float* scales, const float* rotations, const float* view,
                          const int* radii, float* out_gauss_normals, hipStream_t s)
{
    if (P <= 0) return;
    const dim3 grid((unsigned)((P + 255) / 256)), block(256);
    float4* out = reinterpret_cast<float4*>(out_gauss_normals);
    if (raw) hipLaunchKernelGGL((k_gauss_normals<true>), grid, block, 0, s, P, means3D, scales, rotations, view, radii, out);
    else hipLaunchKernelGGL((k_gauss_normals<false>), grid, block, 0, s, P, means3D, scales, rotations, view, radii, out);
}

void launch_render_normals(int W, int H, int P, const GeomView& g, const ImgView& im, const char* bin_base,
                           const float* gauss_normals, float* out_normals, hipStream_t s)
{
    const TileGrid t = tile_grid(W, H);
    if (t.num_tiles <= 0) return;
    if (P <= 0) {                                                     // the forward of an empty cloud wrote no header and no list
        const long long n = 3ll * W * H;
        hipLaunchKernelGGL(k_normals_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, out_normals);
        return;
    }
    dispatch_strict([&](auto st) {
        hipLaunchKernelGGL((k_render_normals<st.value>), dim3(t.grid), dim3(WALK_THREADS), 0, s, W, H, t.gx, t.num_tiles, t.tile_map,
                           im.ranges, bin_base, g.rec, g.header, reinterpret_cast<const float4*>(gauss_normals), out_normals);
    });
}

void launch_normals_bwd(int W, int H, int P, const GeomView& g, const ImgView& im, char* bin_base, const float* dL_dnormals,
                        const float* normals, const float* gauss_normals, hipStream_t s)
{
    const TileGrid t = tile_grid(W, H);
    if (P <= 0 || t.num_tiles <= 0) return;
    dispatch_strict([&](auto st) {
        hipLaunchKernelGGL((k_normals_bwd<st.value>), dim3(t.grid), dim3(WALK_THREADS), 0, s, W, H, t.gx, t.num_tiles, t.tile_map,
                           im.ranges, bin_base, g.rec, g.header, dL_dnormals, normals, reinterpret_cast<const float4*>(gauss_normals));
    });
}

void launch_normal_rot_bwd(int P, bool raw, const float* rotations, const float* view, const int* radii, const GeomView& g,
                           const float* gauss_normals, const float* dL_dgauss_normal, float* dL_drot, hipStream_t s)
{
    if (P <= 0) return;
    const dim3 grid((unsigned)((P + 255) / 256)), block(256);
    const float4* gn = reinterpret_cast<const float4*>(gauss_normals);
    float4* dr = reinterpret_cast<float4*>(dL_drot);
    if (raw) hipLaunchKernelGGL((k_normal_rot_bwd<true>), grid, block, 0, s, P, rotations, view, radii, g.header, gn, dL_dgauss_normal, dr);
    else hipLaunchKernelGGL((k_normal_rot_bwd<false>), grid, block, 0, s, P, rotations, view, radii, g.header, gn, dL_dgauss_normal, dr);
}

}  // namespace lr
