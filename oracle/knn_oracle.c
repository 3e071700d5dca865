/*
 * knn_oracle.c -- CPU restatement of simple-knn's distCUDA2 contract.
 * TEST INFRASTRUCTURE ONLY (see raster_oracle.c header).
 *
 * Contract (KNN/ = /root/reference/submodules/simple-knn/): for every point, the mean of the
 * 3 smallest squared Euclidean distances to OTHER points, written at the point's original
 * index (KNN/simple_knn.cu:147-183, :182; updateKBest<3> :131-145).  The reference's Morton
 * ordering + box pruning is an acceleration structure only; the result is the exact 3-NN mean,
 * so the oracle is the brute-force definition.  Distances are float32, d = dx*dx+dy*dy+dz*dz
 * (KNN/simple_knn.cu:119-129).  When fewer than 3 other points exist the unfilled slots keep
 * FLT_MAX (KNN/simple_knn.cu:160: best initialised to FLT_MAX).
 */
#include <float.h>
#include <stdint.h>

void oracle_dist2(int P, const float* pts, float* out)
{
#pragma omp parallel for schedule(static)
    for (int i = 0; i < P; i++) {
        float best[3] = { FLT_MAX, FLT_MAX, FLT_MAX };
        float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        for (int j = 0; j < P; j++) {
            if (j == i) continue;
            float dx = pts[3 * j] - px, dy = pts[3 * j + 1] - py, dz = pts[3 * j + 2] - pz;
            float d = dx * dx + dy * dy + dz * dz;
            /* updateKBest<3>: insertion keeping ascending order */
            for (int k = 0; k < 3; k++) {
                if (best[k] > d) { float t = best[k]; best[k] = d; d = t; }
            }
        }
        out[i] = (best[0] + best[1] + best[2]) / 3.0f;
    }
}

/*
 * Companions of oracle_dist2 for the distCUDA2 tests (tests/test_knn_oracle_cpu.py, tests/test_gpu_knn.py).  oracle_dist2 above
 * is pinned bit for bit to the compiled reference and stays as it is; everything below is the same brute-force loop with one
 * thing changed at a time.
 *
 *   mode 0: float32, d = dx*dx + dy*dy + dz*dz in source order, no contraction (what oracle_dist2 computes)
 *   mode 1: float32, d = fmaf(dz, dz, fmaf(dy, dy, dx*dx))   -- the two ways a compiler that contracts may associate
 *   mode 2: float32, d = fmaf(dz, dz, fmaf(dx, dx, dy*dy))      (dx*dx + dy*dy) + dz*dz: either product of the inner sum stays
 *                                                               a plain multiply, the other two become FMAs
 * A "subset" call evaluates the nq query rows listed in qidx only (out[q] belongs to point qidx[q]); qidx == NULL means all rows.
 */
#include <math.h>
#include <stddef.h>

#if defined(__x86_64__) && defined(__GNUC__) && !defined(__clang__)
/* -ffp-contract=off keeps the plain arithmetic uncontracted; the explicit fmaf calls become one instruction in the clone */
#define KNN_CLONES __attribute__((target_clones("fma", "default")))
#else
#define KNN_CLONES
#endif

KNN_CLONES
static void dist2_f32(int P, const float* pts, int nq, const int* qidx, int mode, float* out)
{
#pragma omp parallel for schedule(static)
    for (int q = 0; q < nq; q++) {
        const int i = qidx ? qidx[q] : q;
        float best[3] = { FLT_MAX, FLT_MAX, FLT_MAX };
        float px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
        for (int j = 0; j < P; j++) {
            if (j == i) continue;
            float dx = pts[3 * (size_t)j] - px, dy = pts[3 * (size_t)j + 1] - py, dz = pts[3 * (size_t)j + 2] - pz;
            float d;
            if (mode == 1) d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            else if (mode == 2) d = fmaf(dz, dz, fmaf(dx, dx, dy * dy));
            else d = dx * dx + dy * dy + dz * dz;
            if (!(best[2] > d)) continue;                 /* the insertion below changes nothing then */
            for (int k = 0; k < 3; k++) {
                if (best[k] > d) { float t = best[k]; best[k] = d; d = t; }
            }
        }
        out[q] = (best[0] + best[1] + best[2]) / 3.0f;
    }
}

void oracle_dist2_subset(int P, const float* pts, int nq, const int* qidx, float* out) { dist2_f32(P, pts, nq, qidx, 0, out); }

/* variant 1 or 2 (see above); qidx == NULL: all P rows (nq is ignored) */
void oracle_dist2_fma(int P, const float* pts, int nq, const int* qidx, int variant, float* out)
{
    dist2_f32(P, pts, qidx ? nq : P, qidx, variant == 2 ? 2 : 1, out);
}

/* The plain high-precision reference: differences, squares, sums and the mean in double on the float32 inputs.  Unfilled slots
 * (fewer than 3 other points) hold FLT_MAX as in the contract; two of them overflow the float32 sum, so the row is +inf, and one
 * of them gives (d0 + d1 + FLT_MAX) / 3. */
void oracle_dist2_f64(int P, const float* pts, int nq, const int* qidx, double* out)
{
    if (!qidx) nq = P;
#pragma omp parallel for schedule(static)
    for (int q = 0; q < nq; q++) {
        const int i = qidx ? qidx[q] : q;
        double best[3] = { FLT_MAX, FLT_MAX, FLT_MAX };
        double px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
        for (int j = 0; j < P; j++) {
            if (j == i) continue;
            double dx = pts[3 * (size_t)j] - px, dy = pts[3 * (size_t)j + 1] - py, dz = pts[3 * (size_t)j + 2] - pz;
            double d = dx * dx + dy * dy + dz * dz;
            if (!(best[2] > d)) continue;
            for (int k = 0; k < 3; k++) {
                if (best[k] > d) { double t = best[k]; best[k] = d; d = t; }
            }
        }
        out[q] = (best[1] == (double)FLT_MAX) ? INFINITY : (best[0] + best[1] + best[2]) / 3.0;
    }
}
