// project_point.h -- the float64 projection of one cloud point, shared by reproject.hip and dream.hip so that both form the
// same bits: p = R x + T, q = K p, u = q0 / q2, v = q1 / q2, every row ((a0 x + a1 y) + a2 z) + t, one IEEE operation each.
// Both translation units are compiled with -ffp-contract=off (include/lucid_raster.h, lr_reproject).
#pragma once
#include "common.h"

namespace lr {

struct Cameras {
    double K[9];
    double R[REPROJECT_FRAMES_PER_LAUNCH][9];
    double T[REPROJECT_FRAMES_PER_LAUNCH][3];
};

struct Projected {
    double u, v;
    float z;
    int iu, iv;
    bool valid;
};

__device__ __forceinline__ double row3(const double* m, double a, double b, double c) { return (m[0] * a + m[1] * b) + m[2] * c; }

__device__ __forceinline__ Projected project_point(const Cameras& cam, int f, const float* __restrict__ pts, long long ps,
                                                   long long cs, int i, int W, int H)
{
    const double x = (double)pts[(size_t)i * ps], y = (double)pts[(size_t)i * ps + cs], z = (double)pts[(size_t)i * ps + 2 * cs];
    const double p0 = row3(cam.R[f], x, y, z) + cam.T[f][0];
    const double p1 = row3(cam.R[f] + 3, x, y, z) + cam.T[f][1];
    const double p2 = row3(cam.R[f] + 6, x, y, z) + cam.T[f][2];
    const double q0 = row3(cam.K, p0, p1, p2), q1 = row3(cam.K + 3, p0, p1, p2), q2 = row3(cam.K + 6, p0, p1, p2);
    Projected r;
    r.u = q0 / q2;
    r.v = q1 / q2;
    // NaN fails every comparison
    r.valid = q2 > 0.0 && r.u >= 0.0 && r.u <= (double)(W - 1) && r.v >= 0.0 && r.v <= (double)(H - 1);
    r.iu = r.valid ? (int)rint(r.u) : 0;        // round half to even, as np.round
    r.iv = r.valid ? (int)rint(r.v) : 0;
    r.z = (float)q2;
    return r;
}

}  // namespace lr
