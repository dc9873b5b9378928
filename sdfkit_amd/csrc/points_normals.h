// points_normals.h -- the arithmetic of point-cloud normals and of point clouds as signed distance volumes (lib_pointcloud.hip),
// written once for the device and the host: covariance of a neighbourhood, the symmetric 3x3 eigen step, orientation, the blend
// of tangent-plane distances.  Plain C++ outside hipcc, so that tests/cpp/points_normals_host.cpp checks it as the kernels run
// it; tests/pointcloud_model.py restates it in numpy.  Contract: include/sdfkit_hip.h, "Point clouds: normals and volumes".
//
// Everything here is binary64 from the f32 inputs, one rounding per written operation, in the order written (-ffp-contract=off),
// + - * / and sqrt only (all correctly rounded), and one final rounding to f32 per result.
#pragma once
#include "points_knn.h"

#define SDFK_PC_HD SDFK_KNN_HD

namespace sdfk_pc {

constexpr int kMinNormalK = 3;
constexpr int kSweeps = 8;   // cyclic Jacobi sweeps, fixed: a 3x3 converges to binary64 precision in 5 or 6

// ---- covariance ----------------------------------------------------------------------------------------------------------------
// The neighbours p_j (j = 0 .. m-1, in (d2, index) order) of the point p_i, as differences q_j = (double)p_j - (double)p_i per
// component.  Pass 1: sum += q_j per component, in order; mean = sum / (double)m.  Pass 2: d = q_j - mean; the six sums
// c00 += d0 d0, c01 += d0 d1, c02 += d0 d2, c11 += d1 d1, c12 += d1 d2, c22 += d2 d2, in order.  (The sums are not divided by m:
// neither the eigenvectors nor the ratio of eigenvalues depends on the scale.)
struct Mean {
    double s[3] = {0.0, 0.0, 0.0};
    SDFK_PC_HD void add(const float p[3], const float pi[3])
    {
        for (int a = 0; a < 3; a++) s[a] += (double)p[a] - (double)pi[a];
    }
    SDFK_PC_HD void finish(int m)
    {
        for (int a = 0; a < 3; a++) s[a] = s[a] / (double)m;
    }
};
struct Cov {
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
    SDFK_PC_HD void add(const float p[3], const float pi[3], const Mean& mean)
    {
        const double d0 = ((double)p[0] - (double)pi[0]) - mean.s[0];
        const double d1 = ((double)p[1] - (double)pi[1]) - mean.s[1];
        const double d2 = ((double)p[2] - (double)pi[2]) - mean.s[2];
        c00 += d0 * d0; c01 += d0 * d1; c02 += d0 * d2;
        c11 += d1 * d1; c12 += d1 * d2; c22 += d2 * d2;
    }
    SDFK_PC_HD double trace() const { return (c00 + c11) + c22; }
};

// ---- eigenvectors ----------------------------------------------------------------------------------------------------------------
// Cyclic Jacobi on the symmetric A (a[p][q], upper triangle kept in both halves), V = I at the start; kSweeps sweeps, each over the
// pairs (0,1), (0,2), (1,2).  A pair whose a_pq is exactly 0 is skipped.  Otherwise, with r the third index:
//   theta = (a_qq - a_pp) / (2 a_pq);  t = 1 / (|theta| + sqrt(theta theta + 1)), negated when theta < 0;
//   c = 1 / sqrt(t t + 1);  s = t c;
//   a_pp' = a_pp - t a_pq;  a_qq' = a_qq + t a_pq;  a_pq' = 0;
//   a_rp' = c a_rp - s a_rq;  a_rq' = s a_rp + c a_rq;
//   for each row k of V:  v_kp' = c v_kp - s v_kq;  v_kq' = s v_kp + c v_kq.
// (theta theta may overflow to +inf for a tiny a_pq: then t = 0, c = 1, s = 0 and the pair is left as it is.)
// Afterwards the eigenvalues are the diagonal, the eigenvectors the columns of V.
struct Eigen3 {
    double a[3][3];
    double v[3][3];
    template <int p, int q, int r>
    SDFK_PC_HD void rotate()
    {
        const double apq = a[p][q];
        if (apq == 0.0) return;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double at = theta < 0.0 ? -theta : theta;
        double t = 1.0 / (at + __builtin_sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
        const double s = t * c;
        a[p][p] = a[p][p] - t * apq;
        a[q][q] = a[q][q] + t * apq;
        a[p][q] = a[q][p] = 0.0;
        const double arp = a[r][p], arq = a[r][q];
        a[r][p] = a[p][r] = c * arp - s * arq;
        a[r][q] = a[q][r] = s * arp + c * arq;
        for (int k = 0; k < 3; k++) {
            const double vkp = v[k][p], vkq = v[k][q];
            v[k][p] = c * vkp - s * vkq;
            v[k][q] = s * vkp + c * vkq;
        }
    }
    SDFK_PC_HD void solve(const Cov& C)
    {
        a[0][0] = C.c00; a[0][1] = a[1][0] = C.c01; a[0][2] = a[2][0] = C.c02;
        a[1][1] = C.c11; a[1][2] = a[2][1] = C.c12; a[2][2] = C.c22;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
        for (int sweep = 0; sweep < kSweeps; sweep++) {
            rotate<0, 1, 2>();
            rotate<0, 2, 1>();
            rotate<1, 2, 0>();
        }
    }
    // the column of the least eigenvalue, ties to the lowest column
    SDFK_PC_HD int least(double* lmin) const
    {
        int col = 0;
        *lmin = a[0][0];
        if (a[1][1] < *lmin) { col = 1; *lmin = a[1][1]; }
        if (a[2][2] < *lmin) { col = 2; *lmin = a[2][2]; }
        return col;
    }
};

// ---- one point's normal --------------------------------------------------------------------------------------------------------
// From the finished covariance of m neighbours: degenerate (m < 3 or trace == 0): normal = (0, 0, 0), variation = 0.  Otherwise
// n = column least() of V, normalised: len = sqrt((n0 n0 + n1 n1) + n2 n2), n_a = n_a / len; oriented (below); normal = (float)n_a;
// variation = (float)(max(l_min, 0) / ((l_0 + l_1) + l_2)), l the diagonal after the sweeps: the covariance is positive semi-definite, so
// an l_min below zero is rounding noise (every exactly planar neighbourhood, three points among them) and counts as zero.
// Orientation.  With a viewpoint w: d = ((w0 - p0) n0 + (w1 - p1) n1) + (w2 - p2) n2 (binary64, w and p widened first); d < 0
// flips n, d > 0 keeps it.  Without a viewpoint, or when d is neither (exactly 0, or NaN from a non-finite viewpoint of the
// unchecked device form): the component of largest magnitude is made positive, ties to the lowest axis.
SDFK_PC_HD void normal_of(const Cov& C, int m, const float pi[3], bool has_viewpoint, const float viewpoint[3], float normal[3], float* variation)
{
    normal[0] = normal[1] = normal[2] = 0.0f;
    *variation = 0.0f;
    if (m < kMinNormalK || C.trace() == 0.0) return;
    Eigen3 E;
    E.solve(C);
    double lmin;
    const int col = E.least(&lmin);
    double n[3];
    for (int a = 0; a < 3; a++) n[a] = col == 0 ? E.v[a][0] : (col == 1 ? E.v[a][1] : E.v[a][2]);
    const double len = __builtin_sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    for (int a = 0; a < 3; a++) n[a] = n[a] / len;
    bool flip = false, decided = false;
    if (has_viewpoint) {
        const double d = (((double)viewpoint[0] - (double)pi[0]) * n[0] + ((double)viewpoint[1] - (double)pi[1]) * n[1]) +
                         ((double)viewpoint[2] - (double)pi[2]) * n[2];
        decided = d < 0.0 || d > 0.0;
        flip = d < 0.0;
    }
    if (!decided) {
        double big = n[0], mag = n[0] < 0.0 ? -n[0] : n[0];
        for (int a = 1; a < 3; a++) {
            const double ma = n[a] < 0.0 ? -n[a] : n[a];
            if (ma > mag) { mag = ma; big = n[a]; }
        }
        flip = big < 0.0;
    }
    for (int a = 0; a < 3; a++) normal[a] = (float)(flip ? -n[a] : n[a]);
    if (lmin < 0.0) lmin = 0.0;
    *variation = (float)(lmin / ((E.a[0][0] + E.a[1][1]) + E.a[2][2]));
}

// ---- the volume: a blend of tangent-plane distances ------------------------------------------------------------------------------
// At the point x with neighbours (p_j, n_j, d2_j) in order, h2 the cut-off (the d2 of neighbour k - 1 when k were found, else the
// radius bound of max_distance).  A neighbour whose normal is (0, 0, 0) (either sign of zero) is skipped.  For the others
//   e_j = ((x0 - p0) n0 + (x1 - p1) n1) + (x2 - p2) n2   (binary64, every float widened first),
//   and, when h2 > 0:  t = (double)d2_j / (double)h2,  u = 1 - t,  w = u u,  S += w e_j,  W += w.
// value = S / W when W > 0, else e of the first unskipped neighbour (k = 1, h2 == 0, every d2 equal to h2).  No unskipped
// neighbour: the voxel is unknown.  The value is rounded to f32, then clamped to [-max_distance, max_distance].
struct Blend {
    double S = 0.0, W = 0.0, first = 0.0;
    bool any = false;
    SDFK_PC_HD void add(const float x[3], const float p[3], const float n[3], float d2, float h2)
    {
        if (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) return;
        const double e = (((double)x[0] - (double)p[0]) * (double)n[0] + ((double)x[1] - (double)p[1]) * (double)n[1]) +
                         ((double)x[2] - (double)p[2]) * (double)n[2];
        if (!any) { first = e; any = true; }
        if (h2 > 0.0f) {
            const double t = (double)d2 / (double)h2;
            const double u = 1.0 - t;
            const double w = u * u;
            S += w * e;
            W += w;
        }
    }
    SDFK_PC_HD bool known() const { return any; }
    SDFK_PC_HD float value(float max_distance) const
    {
        float f = (float)(W > 0.0 ? S / W : first);
        if (f > max_distance) f = max_distance;
        if (f < -max_distance) f = -max_distance;
        return f;
    }
};
// the cut-off: m neighbours found of k asked, `last_d2` the d2 of the m-th
SDFK_PC_HD float cutoff_d2(int m, int k, float last_d2, float d2_bound) { return m == k ? last_d2 : d2_bound; }
// the sign a known voxel hands to the far fill: -1 below zero, +1 otherwise (-0.0 included)
SDFK_PC_HD int sign_of(float value) { return value < 0.0f ? -1 : 1; }

// ---- the far fill ----------------------------------------------------------------------------------------------------------------
// One line of `n` signs (0 unknown, +-1), `stride` apart: every unknown entry takes the last non-zero sign before it, the leading
// ones the first non-zero sign after them; a line without one is left as it is.  Returns whether the line had a sign.
// lib_pointcloud.hip runs it over the lines along z, then y, then x; filled(i, sign) is called for every entry that got one.
template <class F>
SDFK_PC_HD bool fill_line(signed char* sgn, int n, long long stride, F&& filled)
{
    int first = -1;
    for (int i = 0; i < n; i++)
        if (sgn[(long long)i * stride] != 0) { first = i; break; }
    if (first < 0) return false;
    signed char carry = sgn[(long long)first * stride];
    for (int i = 0; i < n; i++) {
        signed char& s = sgn[(long long)i * stride];
        if (s != 0) { carry = s; continue; }
        s = carry;
        filled(i, (int)carry);
    }
    return true;
}

}  // namespace sdfk_pc
