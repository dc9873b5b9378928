// redistance.h -- the arithmetic of Voxels.Redistance (sdfk_volume_redistance): the front value of a voxel next to the
// iso-surface and the first-order Godunov upwind update of the Eikonal equation |grad T| = 1.  Plain C++ for the kernels of
// lib_redistance.hip AND for a host build (tests/cpp/redistance_host.cpp), so that the test checks the code the kernels run.
// Contract: include/sdfkit_hip.h, "Redistancing".  binary64 throughout, every operation in the order written here, no
// contraction (the build's -ffp-contract=off), one rounding to f32 at the end of each function.
#ifndef SDFKIT_REDISTANCE_H
#define SDFKIT_REDISTANCE_H

#include <cmath>

#ifdef __HIPCC__
#define SDFK_RD_HD __host__ __device__ __forceinline__
#else
#define SDFK_RD_HD inline
#endif

namespace sdfk_redistance {

// The tile of the block-active schedule (lib_redistance.hip, and the tile-sweep counts of the model and the host solver).
constexpr int kTile = 8;

SDFK_RD_HD bool rd_outside(double s) { return s > 0.0; }

// Front value.  s = v(x) - iso; sn[2 a + 0 / 1] = v(n) - iso of the neighbour at x - e_a / x + e_a, in[...] = that neighbour is
// in range.  h = cell sizes.  Returns true and *t0 when x is on the front (some in-range neighbour on the other side).
SDFK_RD_HD bool rd_front(double s, const double sn[6], const bool in[6], const double h[3], float* t0)
{
    const bool o = rd_outside(s);
    const double as = __builtin_fabs(s);
    bool front = false, zero = false;
    double sum = 0.0;
    for (int a = 0; a < 3; a++) {
        double t = INFINITY;
        bool has = false;
        for (int side = 0; side < 2; side++) {
            const int j = 2 * a + side;
            if (!in[j] || rd_outside(sn[j]) == o) continue;
            const double c = (h[a] * as) / (as + __builtin_fabs(sn[j]));
            if (!has || c < t) t = c;
            has = true;
        }
        if (!has) continue;
        front = true;
        if (t == 0.0) zero = true;
        sum = sum + 1.0 / (t * t);
    }
    if (!front) return false;
    *t0 = zero ? 0.0f : (float)(1.0 / __builtin_sqrt(sum));
    return true;
}

// Godunov update from the per-axis upwind values a[i] = min(T(x - e_i), T(x + e_i)) (out of range: +inf) and cell sizes h.
SDFK_RD_HD float rd_update(const double a_in[3], const double h_in[3])
{
    // ascending a, ties keep x, y, z order (a stable three-element insertion sort)
    double a[3] = {a_in[0], a_in[1], a_in[2]}, h[3] = {h_in[0], h_in[1], h_in[2]};
    if (a[1] < a[0]) { double t = a[0]; a[0] = a[1]; a[1] = t; t = h[0]; h[0] = h[1]; h[1] = t; }
    if (a[2] < a[1]) {
        double t = a[1]; a[1] = a[2]; a[2] = t; t = h[1]; h[1] = h[2]; h[2] = t;
        if (a[1] < a[0]) { t = a[0]; a[0] = a[1]; a[1] = t; t = h[0]; h[0] = h[1]; h[1] = t; }
    }
    double u = a[0] + h[0];
    if (u > a[1]) {
        const double w0 = 1.0 / (h[0] * h[0]), w1 = 1.0 / (h[1] * h[1]);
        double A = w0 + w1;
        double B = w0 * a[0] + w1 * a[1];
        double S = (w0 * a[0]) * a[0] + (w1 * a[1]) * a[1];
        double D = B * B - A * (S - 1.0);
        u = (B + __builtin_sqrt(D > 0.0 ? D : 0.0)) / A;
        if (u > a[2]) {
            const double w2 = 1.0 / (h[2] * h[2]);
            A = A + w2;
            B = B + w2 * a[2];
            S = S + (w2 * a[2]) * a[2];
            D = B * B - A * (S - 1.0);
            u = (B + __builtin_sqrt(D > 0.0 ? D : 0.0)) / A;
        }
    }
    return (float)u;
}

// One voxel of one sweep.  t = T_k(x) (not frozen), tn[2 a + 0 / 1] = T_k of the neighbours (+inf out of range), band = the
// f32 max_distance: a value above it is not stored (it could only influence values above it: the header's causality note).
SDFK_RD_HD float rd_sweep_voxel(float t, const float tn[6], const double h[3], float band)
{
    double a[3];
    for (int i = 0; i < 3; i++) a[i] = (double)(tn[2 * i] < tn[2 * i + 1] ? tn[2 * i] : tn[2 * i + 1]);
    const float u = rd_update(a, h);
    return (u < t && u <= band) ? u : t;
}

// Result: the clamp and the input's sign (v == iso is inside: -0.0 for a distance of zero).
SDFK_RD_HD float rd_finish(float t, double s, float band)
{
    const float m = t < band ? t : band;
    return rd_outside(s) ? m : -m;
}

}  // namespace sdfk_redistance

#endif
