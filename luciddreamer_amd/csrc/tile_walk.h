// tile_walk.h -- "walk this tile's list as the forward did", once, for the passes that run behind a finished forward
// (render_median.hip, render_distort.hip), for gfx950.
//
// The quadrant shape of k_render_fwd: one 256-thread workgroup per 16x16 tile through the same blend_tile map, a wave owns one 8x8
// quadrant, a lane one pixel.  A round stages what alpha needs of BATCH list entries in LDS (x, y, three conic terms, opacity, one
// value of the pass's choice, the cull threshold, the two slopes of box_hit); lane l culls staged entry sb + l against the wave's
// quadrant with box_hit (the forward's test on the forward's operands: a non-candidate cannot reach alpha >= 1/255 on any pixel of
// the box, so skipping it is exactly a `continue` -- repeating the test instead of reading the forward's quad_hits bytes keeps a
// pass independent of which forward shape left them), and the wave walks the ballot mask in list order, alpha by gauss_row<STRICT> /
// gauss_weight<STRICT> on the staged coefficients (the "strict" knob as it is at the call): the forward's arithmetic in the
// forward's order, so a pass that keeps T as the forward does repeats its decisions bit for bit.  A quadrant leaves the walk when
// every pixel of it is done or the list ends; the workgroup leaves it when every wave has.  The R-dependent offsets of the binning
// buffer are resolved on the device from GeomHeader::bin_bound, as the blend backward does.
//
// What a pass brings (tile_walk's callbacks, all inlined):
//     stage(slot, id, z) -> kept      per staged entry, by thread `slot`: `kept` goes to s_q1[slot].z and comes back to the other two;
//                                     whatever else the pass stages per entry (the median's Gaussian id) it stores itself
//     body(j, kept, alpha, use) -> fin  per candidate, by the whole wave: alpha = min(0.99, opacity G), `use` the pixels not done
//                                     with power <= 0 and alpha >= 1/255; updates the pass's per-pixel state and returns the pixels
//                                     that take no further entry
//     finish(j, kept, fin)            only where fin != 0, before they are added to `done` and `done` is tested: the blend
//                                     forward's nesting, which keeps the candidate loop's common path free of that test
//
// k_distort_bwd (render_distort.hip) has the same shape with a flush at the end of every round.  It shares quad_lane and the launch
// helpers and keeps its loop: on this walker (three more hooks: every wave done, round begins, round ends) it computed the same bits
// and measured 2 % slower on the MI355X (129.4 against 126.8 us on C3).
// The blend pair (render_fwd.hip, render_bwd.hip) is hand-scheduled and does not use this header.
#pragma once
#include "common.h"
#include "dispatch_flags.h"

namespace lr {

constexpr int WALK_THREADS = 256;       // 4 wave64 per tile
constexpr int WALK_WAVES = WALK_THREADS / 64;

// ---- host: the launch of a kernel of this shape -----------------------------------------------------------------------------------
struct TileGrid { int gx, gy, num_tiles, tile_map, grid; };
inline TileGrid tile_grid(int W, int H)
{
    TileGrid t;
    t.gx = (W + TILE_X - 1) / TILE_X; t.gy = (H + TILE_Y - 1) / TILE_Y;
    t.num_tiles = t.gx * t.gy;
    t.tile_map = blend_tile_map(t.num_tiles);
    t.grid = ((t.num_tiles + 7) / 8) * 8;
    return t;
}
// f(strict): called once, strict.value = the "strict" knob as a compile-time constant
template <class F>
void dispatch_strict(F&& f)
{
    dispatch_flags<1>(flag_bits(tune_get(TUNE_STRICT) > 0), f);
}

#if defined(__HIPCC__)
// ---- device -------------------------------------------------------------------------------------------------------------------------
// a lane's place: thread, wave, lane, its pixel and the box of its wave's quadrant
struct QuadLane { int tid, w, l, px, py; bool inside; float pxf, pyf, bx0, bx1, by0, by1; };
__device__ __forceinline__ QuadLane quad_lane(int tile, int gx, int W, int H)
{
    QuadLane q;
    const int tx = tile % gx, ty = tile / gx;
    q.tid = threadIdx.x; q.w = q.tid >> 6; q.l = q.tid & 63;
    const int x0 = tx * TILE_X + (q.w & 1) * 8, y0 = ty * TILE_Y + (q.w >> 1) * 8;
    q.px = x0 + (q.l & 7); q.py = y0 + (q.l >> 3);
    q.inside = q.px < W && q.py < H;
    q.pxf = (float)q.px; q.pyf = (float)q.py;
    q.bx0 = (float)x0; q.bx1 = (float)(x0 + 7); q.by0 = (float)y0; q.by1 = (float)(y0 + 7);
    return q;
}

// A tile's list: `total` entries, Gaussian ids from the tile's first.  An overflowed view's list is truncated: it reads as empty
// (wave-uniform: no barrier is skipped by part of a workgroup).
struct TileList { int total; const uint32_t* list_gid; };
__device__ __forceinline__ TileList tile_list(const GeomHeader* __restrict__ hdr, const uint2* __restrict__ ranges,
                                              const char* __restrict__ bin_base, int tile)
{
    const uint2 range = hdr->overflow != 0u ? make_uint2(0u, 0u) : ranges[tile];
    TileList t;
    t.total = (int)(range.y - range.x);
    t.list_gid = reinterpret_cast<const uint32_t*>(bin_base + bin_layout((long long)hdr->bin_bound).list_gid) + range.x;
    return t;
}

// the staging planes of a walk, __shared__ arrays of the kernel, BATCH entries each (wdone: WALK_WAVES)
struct WalkPlanes {
    float4* q0;         // x, y, Ap, Bp (x log2 e; strict: conic a, b)           -- as k_render_fwd
    float4* q1;         // Cp (strict: conic c), opacity, the pass's value, qmax (cull threshold)
    float2* q2;         // -b/c, -b/a (edge minimiser slopes for box_hit)
    int* wdone;
};

// done: bit l = pixel l of the wave's quadrant takes no entry (the pixels outside the image, at least)
template <bool STRICT, int BATCH, class Stage, class Body, class Finish>
__device__ __forceinline__ void tile_walk(const QuadLane& q, const TileList& tl, const GaussRec* __restrict__ rec,
                                          const WalkPlanes& s, uint64_t done, Stage stage, Body body, Finish finish)
{
    const int tid = q.tid, w = q.w, l = q.l;
    bool wave_done = done == ~0ull;
    for (int base = 0; base < tl.total; base += BATCH) {
        if (l == 0) s.wdone[w] = wave_done ? 1 : 0;
        lds_barrier();                                                // (the previous round is over: its planes may be overwritten)
        if (s.wdone[0] + s.wdone[1] + s.wdone[2] + s.wdone[3] == WALK_WAVES) break;
        const int cnt = min(BATCH, tl.total - base);
        if (tid < cnt) {
            const uint32_t id = tl.list_gid[base + tid];
            const float4* g = reinterpret_cast<const float4*>(rec + id);
            const float4 a = g[0], b = g[1], c = g[2];
            const float kept = stage(tid, id, c.y);
            s.q0[tid] = STRICT ? make_float4(a.x, a.y, a.z, a.w) : make_float4(a.x, a.y, (-0.5f * LOG2E) * a.z, -LOG2E * a.w);
            s.q1[tid] = STRICT ? make_float4(b.x, b.y, kept, c.z) : make_float4((-0.5f * LOG2E) * b.x, b.y, kept, LOG2E * c.z);
            s.q2[tid] = make_float2(-a.w / b.x, -a.w / a.z);
        }
        lds_barrier();
        if (wave_done) continue;

        for (int sb = 0; sb < cnt; sb += 64) {
            bool hit = false;
            const int jl = sb + l;
            if (jl < cnt) {
                const float4 a = s.q0[jl];
                const float4 b = s.q1[jl];
                const float2 r = s.q2[jl];
                const float ca = STRICT ? a.z : -2.0f * a.z, cb = STRICT ? a.w : -a.w, cc = STRICT ? b.x : -2.0f * b.x;
                hit = box_hit(a.x, a.y, ca, cb, cc, r.x, r.y, b.w, q.bx0, q.bx1, q.by0, q.by1);
            }
            uint64_t mask = __ballot(hit);
            while (mask) {
                const int k = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int j = sb + k;
                const float4 a = s.q0[j];
                const float4 b = s.q1[j];
                float r0, r1, power;
                gauss_row<STRICT>(a.w, b.x, a.y - q.pyf, r0, r1);
                const float alpha = fminf(0.99f, b.y * gauss_weight<STRICT>(a.z, a.w, b.x, r0, r1, a.x - q.pxf, power));
                // the forward's order of tests
                const uint64_t use = ~done & __builtin_amdgcn_ballot_w64(power <= 0.0f) & __builtin_amdgcn_ballot_w64(alpha >= 1.0f / 255.0f);
                const uint64_t fin = body(j, b.z, alpha, use);
                if (fin != 0ull) {
                    finish(j, b.z, fin);
                    done |= fin;
                    if (done == ~0ull) break;
                }
            }
            if (done == ~0ull) { wave_done = true; break; }
        }
    }
}
#endif  // __HIPCC__

}  // namespace lr
