// icp_solve.h -- the arithmetic of one IterativeClosestPoint iteration after its reductions (lib_points.hip), written once for the
// device and the host: the piecewise distMax rule and the filter, the 3x3 Kabsch solve (a one-sided Jacobi SVD in binary64), the
// f32 Matrix4x4 product and inverse of System.Numerics, and the composition of step, total and convergence.  Plain C++ outside
// hipcc, so that tests/cpp/icp_solve_host.cpp checks it as the kernels run it; tests/points_model.py (icp_step_exact) restates it in
// numpy.  Contract: include/sdfkit_hip.h, "IterativeClosestPoint.RegisterPoints".
//
// One rounding per written operation, in the order written (-ffp-contract=off), + - * / and sqrt only (all correctly rounded):
// binary64 in dist_max and kabsch_r, binary32 in the distMax rule and the Matrix4x4 part.
#pragma once
#include "points_knn.h"

#define SDFK_ICP_HD SDFK_KNN_HD

namespace sdfk_icp {

// ---- the filter ----------------------------------------------------------------------------------------------------------------
// mean and standard deviation in f64, rounded to f32; distMax in the reference's f32 (IterativeClosestPoint.cs:101-114)
SDFK_ICP_HD float dist_max_rule(float m, float sd, float good)
{
    float dmax;
    if (m < good) dmax = m + 3.0f * sd;
    else if (m < 3.0f * good) dmax = m + 2.0f * sd;
    else if (m < 6.0f * good) dmax = m + sd;
    else dmax = (m + 0.5f) + sd;
    return dmax;
}
// `mean`: the distance mean; `sqsum`: the sum of (d - mean)^2 over the n points
SDFK_ICP_HD float dist_max(double mean, double sqsum, double n, float good)
{
    const float m = (float)mean, sd = (float)__builtin_sqrt(sqsum / n);
    return dist_max_rule(m, sd, good);
}
// a point takes part in the means and in C iff
SDFK_ICP_HD bool kept(float dist, float dmax) { return dist <= dmax; }

// ---- the f32 Matrix4x4 arithmetic of System.Numerics (software forms, as sdfkit_amd/raymarch.py restates them) ----
SDFK_ICP_HD void m4_mul(const float* a, const float* b, float* r)
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            r[4 * i + j] = ((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) + a[4 * i + 3] * b[12 + j];
}

SDFK_ICP_HD bool m4_invert(const float* s, float* R)
{
    const float a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], gq = s[6], h = s[7];
    const float i = s[8], j = s[9], k = s[10], l = s[11], m = s[12], n = s[13], o = s[14], p = s[15];
    const float kp_lo = k * p - l * o, jp_ln = j * p - l * n, jo_kn = j * o - k * n, ip_lm = i * p - l * m, io_km = i * o - k * m, in_jm = i * n - j * m;
    const float a11 = +(f * kp_lo - gq * jp_ln + h * jo_kn), a12 = -(e * kp_lo - gq * ip_lm + h * io_km);
    const float a13 = +(e * jp_ln - f * ip_lm + h * in_jm), a14 = -(e * jo_kn - f * io_km + gq * in_jm);
    const float det = a * a11 + b * a12 + c * a13 + d * a14;
    if (fabsf(det) < 1.1920929e-07f) {
        for (int q = 0; q < 16; q++) R[q] = sdfk_knn::bits_f32(0x7fc00000u);
        return false;
    }
    const float inv = 1.0f / det;
    R[0] = a11 * inv; R[4] = a12 * inv; R[8] = a13 * inv; R[12] = a14 * inv;
    R[1] = -(b * kp_lo - c * jp_ln + d * jo_kn) * inv; R[5] = +(a * kp_lo - c * ip_lm + d * io_km) * inv;
    R[9] = -(a * jp_ln - b * ip_lm + d * in_jm) * inv; R[13] = +(a * jo_kn - b * io_km + c * in_jm) * inv;
    const float gp_ho = gq * p - h * o, fp_hn = f * p - h * n, fo_gn = f * o - gq * n, ep_hm = e * p - h * m, eo_gm = e * o - gq * m, en_fm = e * n - f * m;
    R[2] = +(b * gp_ho - c * fp_hn + d * fo_gn) * inv; R[6] = -(a * gp_ho - c * ep_hm + d * eo_gm) * inv;
    R[10] = +(a * fp_hn - b * ep_hm + d * en_fm) * inv; R[14] = -(a * fo_gn - b * eo_gm + c * en_fm) * inv;
    const float gl_hk = gq * l - h * k, fl_hj = f * l - h * j, fk_gj = f * k - gq * j, el_hi = e * l - h * i, ek_gi = e * k - gq * i, ej_fi = e * j - f * i;
    R[3] = -(b * gl_hk - c * fl_hj + d * fk_gj) * inv; R[7] = +(a * gl_hk - c * el_hi + d * ek_gi) * inv;
    R[11] = -(a * fl_hj - b * el_hi + d * ej_fi) * inv; R[15] = +(a * fk_gj - b * ek_gi + c * ej_fi) * inv;
    return true;
}

// ---- the solve -----------------------------------------------------------------------------------------------------------------
SDFK_ICP_HD uint64_t f64_bits(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return u;
}
SDFK_ICP_HD double bits_f64(uint64_t u)
{
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
}

// The power of two that brings the largest |C_ab| into [1, 2), as two factors (one alone is not always a normal number): every
// product C_ab * f1 * f2 is exact.  C = 0 or a non-finite largest magnitude: 1, 1.  R does not depend on the scale of C, but
// al * be below grows like its fourth power and would overflow for |C| above 2^256 (and underflow below 2^-256).
SDFK_ICP_HD void pow2_scale(const double C[9], double* f1, double* f2)
{
    double m = 0.0;
    for (int q = 0; q < 9; q++) {
        const double a = fabs(C[q]);
        if (a > m) m = a;
    }
    *f1 = 1.0;
    *f2 = 1.0;
    if (!(m > 0.0) || !(m < (double)INFINITY)) return;
    if (m < 0x1p-1022) *f1 = 0x1p+1022;     // subnormal: into [2^-52, 1)
    else if (m >= 0x1p+1023) *f1 = 0.5;
    const int e = (int)((f64_bits(m * *f1) >> 52) & 0x7ff) - 1023;   // in [-1022, 1022]
    *f2 = bits_f64((uint64_t)(1023 - e) << 52);
}

// C = U S V^T (f64, one-sided Jacobi on the columns of C); returns R = V diag(1, 1, sign det(V U^T)) U^T.  U and V are
// orthogonal whatever the rank: u3 = u1 x u2 (R does not depend on the sign of u3: det(V U^T) flips with it), and u2 is
// completed with a cross product when sigma2 vanishes.
SDFK_ICP_HD void kabsch_r(const double C[9], double R[9])
{
    double W[3][3], V[3][3];   // W = C V, columns orthogonalised
    double f1, f2;
    pow2_scale(C, &f1, &f2);
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) { W[a][b] = (C[3 * a + b] * f1) * f2; V[a][b] = a == b ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int i = 0; i < 2; i++)
            for (int j = i + 1; j < 3; j++) {
                double al = 0, be = 0, ga = 0;
                for (int k = 0; k < 3; k++) { al += W[k][i] * W[k][i]; be += W[k][j] * W[k][j]; ga += W[k][i] * W[k][j]; }
                if (ga == 0.0 || fabs(ga) <= 1e-15 * __builtin_sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + __builtin_sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / __builtin_sqrt(1.0 + t * t), sn = cs * t;
                for (int k = 0; k < 3; k++) {
                    const double wi = W[k][i], wj = W[k][j];
                    W[k][i] = cs * wi - sn * wj; W[k][j] = sn * wi + cs * wj;
                    const double vi = V[k][i], vj = V[k][j];
                    V[k][i] = cs * vi - sn * vj; V[k][j] = sn * vi + cs * vj;
                }
            }
        if (!rotated) break;
    }
    double sg[3];
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 3; i++) sg[i] = __builtin_sqrt(W[0][i] * W[0][i] + W[1][i] * W[1][i] + W[2][i] * W[2][i]);
    for (int i = 0; i < 2; i++)   // descending singular values
        for (int j = 0; j < 2 - i; j++)
            if (sg[ord[j]] < sg[ord[j + 1]]) { const int t = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = t; }
    double U[3][3], Vs[3][3];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) Vs[k][i] = V[k][ord[i]];
    const double s0 = sg[ord[0]], s1 = sg[ord[1]];
    if (s0 == 0.0) {   // C = 0: U = V = I
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) { U[a][b] = a == b; Vs[a][b] = a == b; }
    } else {
        for (int k = 0; k < 3; k++) U[k][0] = W[k][ord[0]] / s0;
        if (s1 > 1e-12 * s0) {
            for (int k = 0; k < 3; k++) U[k][1] = W[k][ord[1]] / s1;
        } else {   // any unit vector orthogonal to u1
            const double ax = fabs(U[0][0]), ay = fabs(U[1][0]), az = fabs(U[2][0]);
            double e[3] = {0, 0, 0};
            e[ax <= ay && ax <= az ? 0 : (ay <= az ? 1 : 2)] = 1.0;
            double w[3] = {U[1][0] * e[2] - U[2][0] * e[1], U[2][0] * e[0] - U[0][0] * e[2], U[0][0] * e[1] - U[1][0] * e[0]};
            const double l = __builtin_sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            for (int k = 0; k < 3; k++) U[k][1] = w[k] / l;
        }
        U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
        U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
        U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    }
    // sign det(V U^T) = sign det V * det U, det U = +1 by construction
    const double detv = Vs[0][0] * (Vs[1][1] * Vs[2][2] - Vs[1][2] * Vs[2][1]) - Vs[0][1] * (Vs[1][0] * Vs[2][2] - Vs[1][2] * Vs[2][0]) +
                        Vs[0][2] * (Vs[1][0] * Vs[2][1] - Vs[1][1] * Vs[2][0]);
    const double d3 = detv > 0 ? 1.0 : (detv < 0 ? -1.0 : 0.0);
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) R[3 * a + b] = Vs[a][0] * U[b][0] + Vs[a][1] * U[b][1] + d3 * Vs[a][2] * U[b][2];
}

// ---- one iteration's step ------------------------------------------------------------------------------------------------------
// From C, the filtered means and the running total: R (kabsch_r), R, pmean and qmean rounded to f32, then the reference's f32 steps:
// translation = Transform(pmean, Invert(R)) - qmean, step = Invert(R * CreateTranslation(t)), convergence on the step
// (IterativeClosestPoint.cs:66-69), total = total * step (:72).  `total_prev` and `total` may not overlap.
SDFK_ICP_HD void solve_step(const double C[9], const double pmean[3], const double qmean[3], const float total_prev[16], float conv_t, float conv_r,
                            float step[16], float total[16], bool* converged)
{
    double Rd[9];
    kabsch_r(C, Rd);
    float rm[16] = {(float)Rd[0], (float)Rd[1], (float)Rd[2], 0, (float)Rd[3], (float)Rd[4], (float)Rd[5], 0,
                    (float)Rd[6], (float)Rd[7], (float)Rd[8], 0, 0, 0, 0, 1};
    const float pm[3] = {(float)pmean[0], (float)pmean[1], (float)pmean[2]};
    const float qm[3] = {(float)qmean[0], (float)qmean[1], (float)qmean[2]};
    float inv_r[16], tm[16], xf[16];
    m4_invert(rm, inv_r);
    float tr[3];
    for (int j = 0; j < 3; j++)   // Vector3.Transform(pmean, invR) - qmean
        tr[j] = (((pm[0] * inv_r[j] + pm[1] * inv_r[4 + j]) + pm[2] * inv_r[8 + j]) + inv_r[12 + j]) - qm[j];
    for (int q = 0; q < 16; q++) tm[q] = (q % 5 == 0) ? 1.0f : 0.0f;
    tm[12] = tr[0]; tm[13] = tr[1]; tm[14] = tr[2];
    m4_mul(rm, tm, xf);
    m4_invert(xf, step);
    const float drot = (fabsf(1.0f - step[0]) + fabsf(1.0f - step[5])) + fabsf(1.0f - step[10]);
    const float dtrans = (float)__builtin_sqrt((double)((step[12] * step[12] + step[13] * step[13]) + step[14] * step[14]));   // Vector3.Length
    *converged = dtrans <= conv_t && drot <= conv_r;
    m4_mul(total_prev, step, total);
}

}  // namespace sdfk_icp

// ---- point to plane ------------------------------------------------------------------------------------------------------------
// The second metric (contract: include/sdfkit_hip.h, "IterativeClosestPoint.RegisterPoints, point to plane"): the distance to the
// tangent plane at the nearest static point is minimised.  With R = I + [omega]x about the kept points' mean and a translation t,
// the residual of a kept point is r + J . (omega, t), J = (d x n, n), d = p - pmean, r = (p - q) . n; the kernels reduce
// A = sum J J^T and b = sum J r, and everything after that is here.  tests/cpp/icp_plane_host.cpp checks it on the host and
// tests/icp_plane_model.py restates it in numpy.  Binary64 throughout, one rounding per written operation.
namespace sdfk_icp {

constexpr int kSweeps6 = 8;            // cyclic Jacobi sweeps on the 6x6, fixed (x stops changing after 6, rarely 7)
constexpr double kPlaneTau = 1e-12;    // eigenvalues at or below kPlaneTau * lambda_max are unobserved directions: no step along them

// a correspondence takes part iff it exists, passes the distance filter and its static normal is not (0, 0, 0)
SDFK_ICP_HD bool kept_plane(int index, float dist, float dmax, const float n[3])
{
    return index >= 0 && kept(dist, dmax) && !(n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f);
}

// one kept point: the row J and the residual r
SDFK_ICP_HD void plane_row(const float p[3], const float q[3], const float n[3], const double pmean[3], double J[6], double* r)
{
    const double p0 = (double)p[0], p1 = (double)p[1], p2 = (double)p[2];
    const double n0 = (double)n[0], n1 = (double)n[1], n2 = (double)n[2];
    const double d0 = p0 - pmean[0], d1 = p1 - pmean[1], d2 = p2 - pmean[2];
    J[0] = d1 * n2 - d2 * n1; J[1] = d2 * n0 - d0 * n2; J[2] = d0 * n1 - d1 * n0;
    J[3] = n0; J[4] = n1; J[5] = n2;
    *r = ((p0 - (double)q[0]) * n0 + (p1 - (double)q[1]) * n1) + (p2 - (double)q[2]) * n2;
}

// Cyclic Jacobi on the symmetric 6x6 A, the conventions of points_normals.h's Eigen3 widened: V = I at the start; kSweeps6 sweeps,
// each over the pairs (p, q), p < q, in row order (0,1), (0,2), ..., (0,5), (1,2), ..., (4,5).  A pair whose a_pq is exactly 0 is
// skipped.  Otherwise theta = (a_qq - a_pp) / (2 a_pq);  t = 1 / (|theta| + sqrt(theta theta + 1)), negated when theta < 0;
// c = 1 / sqrt(t t + 1);  s = t c;  a_pp' = a_pp - t a_pq;  a_qq' = a_qq + t a_pq;  a_pq' = 0;  for every other index r in
// ascending order a_rp' = c a_rp - s a_rq, a_rq' = s a_rp + c a_rq;  for each row k of V: v_kp' = c v_kp - s v_kq,
// v_kq' = s v_kp + c v_kq.  Afterwards the eigenvalues are the diagonal, the eigenvectors the columns of V.
// (Every index is a compile-time constant after unrolling, so that the device keeps both matrices in registers.)
struct Eigen6 {
    double a[6][6];
    double v[6][6];
    template <int p, int q>
    SDFK_ICP_HD void rotate()
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
#pragma unroll
        for (int r = 0; r < 6; r++) {
            if (r == p || r == q) continue;
            const double arp = a[r][p], arq = a[r][q];
            a[r][p] = a[p][r] = c * arp - s * arq;
            a[r][q] = a[q][r] = s * arp + c * arq;
        }
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const double vkp = v[k][p], vkq = v[k][q];
            v[k][p] = c * vkp - s * vkq;
            v[k][q] = s * vkp + c * vkq;
        }
    }
    SDFK_ICP_HD void sweep()
    {
        rotate<0, 1>(); rotate<0, 2>(); rotate<0, 3>(); rotate<0, 4>(); rotate<0, 5>();
        rotate<1, 2>(); rotate<1, 3>(); rotate<1, 4>(); rotate<1, 5>();
        rotate<2, 3>(); rotate<2, 4>(); rotate<2, 5>();
        rotate<3, 4>(); rotate<3, 5>();
        rotate<4, 5>();
    }
};

// A21: the upper triangle of A in row order, (0,0), (0,1), ..., (0,5), (1,1), ..., (5,5)
SDFK_ICP_HD void jacobi6(const double A21[21], Eigen6& E)
{
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) { E.a[i][j] = E.a[j][i] = A21[k]; k++; }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) E.v[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps6; sweep++) E.sweep();
}

// x = sum_k v_k (v_k . (-b)) / lambda_k over the eigenpairs with lambda_k > kPlaneTau lambda_max, k ascending: the least-squares
// solution of A x = -b of least norm, with the directions the correspondences do not observe left at zero.  lambda_max = the
// largest diagonal entry after the sweeps; when it is not a positive finite number (A = 0, or NaN / infinity got in), x = 0 and
// nothing is retained.  Per retained k: dot = 0.0, then dot += v_ak (-b_a) for a = 0 .. 5;  coef = dot / lambda_k;
// x_a += v_ak coef (x = 0.0 at first).  Returns the number of retained eigenvalues; lam receives the six eigenvalues.
SDFK_ICP_HD int pinv_solve6(const double A21[21], const double b[6], double x[6], double lam[6])
{
    Eigen6 E;
    jacobi6(A21, E);
    double nb[6];
#pragma unroll
    for (int a = 0; a < 6; a++) { x[a] = 0.0; nb[a] = -b[a]; lam[a] = E.a[a][a]; }
    double lmax = lam[0];
#pragma unroll
    for (int k = 1; k < 6; k++)
        if (lam[k] > lmax) lmax = lam[k];
    if (!(lmax > 0.0) || !(lmax < (double)INFINITY)) return 0;
    const double cut = kPlaneTau * lmax;
    int retained = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        if (!(lam[k] > cut)) continue;
        retained++;
        double dot = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) dot += E.v[a][k] * nb[a];
        const double coef = dot / lam[k];
#pragma unroll
        for (int a = 0; a < 6; a++) x[a] += E.v[a][k] * coef;
    }
    return retained;
}

// Cayley's rotation of w = x[0..2] / 2 -- exactly orthogonal in exact arithmetic, + - * / only, the rotation by 2 atan |w| about w,
// which agrees with the linearised omega = x[0..2] to second order:  R = ((1 - w.w) I + 2 w w^T + 2 [w]x) / (1 + w.w), with
// ww = (w0 w0 + w1 w1) + w2 w2;  R_aa = ((1 - ww) + 2 (w_a w_a)) / (1 + ww);  R_ab = (2 (w_a w_b) -+ 2 w_c) / (1 + ww), minus for
// (a, b) = (0,1), (1,2), (2,0).  T_a = (pmean_a + x_{3+a}) - ((R_a0 pmean_0 + R_a1 pmean_1) + R_a2 pmean_2): the rotation is about pmean.
SDFK_ICP_HD void cayley_step(const double x[6], const double pmean[3], double R[9], double T[3])
{
    const double w0 = x[0] / 2.0, w1 = x[1] / 2.0, w2 = x[2] / 2.0;
    const double ww = (w0 * w0 + w1 * w1) + w2 * w2;
    const double om = 1.0 - ww, den = 1.0 + ww;
    R[0] = (om + 2.0 * (w0 * w0)) / den;
    R[4] = (om + 2.0 * (w1 * w1)) / den;
    R[8] = (om + 2.0 * (w2 * w2)) / den;
    R[1] = (2.0 * (w0 * w1) - 2.0 * w2) / den;
    R[3] = (2.0 * (w0 * w1) + 2.0 * w2) / den;
    R[2] = (2.0 * (w0 * w2) + 2.0 * w1) / den;
    R[6] = (2.0 * (w0 * w2) - 2.0 * w1) / den;
    R[5] = (2.0 * (w1 * w2) - 2.0 * w0) / den;
    R[7] = (2.0 * (w1 * w2) + 2.0 * w0) / den;
    for (int a = 0; a < 3; a++) T[a] = (pmean[a] + x[3 + a]) - ((R[3 * a] * pmean[0] + R[3 * a + 1] * pmean[1]) + R[3 * a + 2] * pmean[2]);
}

// From the reduced A and b, the kept points' mean and the running total: x (pinv_solve6), R and T (cayley_step) rounded to f32 into the
// row-vector step (R^T in its upper 3x3, T in its fourth row: Transform(p, step) = R p + T), then convergence on the step and
// total = total * step exactly as solve_step.  `total_prev` and `total` may not overlap.
SDFK_ICP_HD void solve_step_plane(const double A21[21], const double b[6], const double pmean[3], const float total_prev[16], float conv_t, float conv_r,
                                  float step[16], float total[16], bool* converged, int* retained)
{
    double x[6], lam[6], R[9], T[3];
    *retained = pinv_solve6(A21, b, x, lam);
    cayley_step(x, pmean, R, T);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) step[4 * i + j] = (float)R[3 * j + i];
        step[4 * i + 3] = 0.0f;
        step[12 + i] = (float)T[i];
    }
    step[15] = 1.0f;
    const float drot = (fabsf(1.0f - step[0]) + fabsf(1.0f - step[5])) + fabsf(1.0f - step[10]);
    const float dtrans = (float)__builtin_sqrt((double)((step[12] * step[12] + step[13] * step[13]) + step[14] * step[14]));   // Vector3.Length
    *converged = dtrans <= conv_t && drot <= conv_r;
    m4_mul(total_prev, step, total);
}

}  // namespace sdfk_icp
