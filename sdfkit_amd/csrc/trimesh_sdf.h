// trimesh_sdf.h -- the arithmetic of lib_trimesh.hip (signed distance volumes from triangle meshes): the binary64 closest point
// on a triangle, the exact orientation sign of three f32 points in the xy plane with its symbolic perturbation, the column
// inside test, the z of a crossing and the columns of a volume that an interval covers.  Plain C++ outside hipcc, so that
// tests/cpp/trimesh_sdf_host.cpp runs exactly the code the kernels run.  Compiled with -ffp-contract=off everywhere: no
// expression below may be fused.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SDFK_TRI_HD __host__ __device__
#else
#define SDFK_TRI_HD
#endif

namespace sdfk_trimesh_sdf {

struct Closest {
    double d2;           // squared distance from the query to cp, binary64
    double cp[3];        // the closest point, binary64 (callers round it to f32)
    double w[3];         // barycentric weights of a, b, c at cp (w[0] + w[1] + w[2] is 1 up to rounding; 0/1 in vertex regions)
};

// n / d for 0 <= n <= d, 0 when d is not positive (a degenerate denominator): always in [0, 1], never NaN
SDFK_TRI_HD inline double ratio(double n, double d) { return d > 0.0 ? n / d : 0.0; }

SDFK_TRI_HD inline double sq3(const double v[3]) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }

// The closest point of segment a + t (b - a), t in [0, 1]: t = clamp(ap.ab / ab.ab), 0 for a zero-length segment.
SDFK_TRI_HD inline void closest_on_segment(const double p[3], const double a[3], const double b[3], double* t_out, double cp[3], double* d2)
{
    double ab[3], ap[3];
    for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ap[k] = p[k] - a[k]; }
    const double num = (ap[0] * ab[0] + ap[1] * ab[1]) + ap[2] * ab[2];
    const double den = sq3(ab);
    double t = num <= 0.0 ? 0.0 : (num >= den ? 1.0 : ratio(num, den));
    double r[3];
    for (int k = 0; k < 3; k++) { cp[k] = a[k] + ab[k] * t; r[k] = p[k] - cp[k]; }
    *t_out = t;
    *d2 = sq3(r);
}

// The triangle measured as its three edges ab, bc, ca, in that order, the first of least d2 winning.
SDFK_TRI_HD inline Closest closest_on_edges(const double p[3], const double a[3], const double b[3], const double c[3])
{
    Closest R;
    double t, cp[3], d2;
    closest_on_segment(p, a, b, &t, cp, &d2);
    R.d2 = d2; R.cp[0] = cp[0]; R.cp[1] = cp[1]; R.cp[2] = cp[2]; R.w[0] = 1.0 - t; R.w[1] = t; R.w[2] = 0.0;
    closest_on_segment(p, b, c, &t, cp, &d2);
    if (d2 < R.d2) { R.d2 = d2; R.cp[0] = cp[0]; R.cp[1] = cp[1]; R.cp[2] = cp[2]; R.w[0] = 0.0; R.w[1] = 1.0 - t; R.w[2] = t; }
    closest_on_segment(p, c, a, &t, cp, &d2);
    if (d2 < R.d2) { R.d2 = d2; R.cp[0] = cp[0]; R.cp[1] = cp[1]; R.cp[2] = cp[2]; R.w[0] = t; R.w[1] = 0.0; R.w[2] = 1.0 - t; }
    return R;
}

// The closest point of triangle (a, b, c) to p, by Voronoi region (vertex a, b, edge ab, vertex c, edge ac, edge bc, face; the
// classic order of Ericson, "Real-Time Collision Detection" 5.1.5).  Triangles whose area term |ab x ac|^2 is exactly zero, and
// face-region results whose three barycentric numerators are not all >= 0 with a positive sum (possible only for nearly
// degenerate triangles), are measured as their three edges: no division by zero, no NaN, every parameter in [0, 1].
SDFK_TRI_HD inline Closest closest_on_triangle(const double p[3], const double a[3], const double b[3], const double c[3])
{
    double ab[3], ac[3], ap[3], bp[3], cq[3];
    for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cq[k] = p[k] - c[k]; }
    const double n0 = ab[1] * ac[2] - ab[2] * ac[1], n1 = ab[2] * ac[0] - ab[0] * ac[2], n2 = ab[0] * ac[1] - ab[1] * ac[0];
    const double area = (n0 * n0 + n1 * n1) + n2 * n2;
    if (area == 0.0) return closest_on_edges(p, a, b, c);
    Closest R;
    double u = 1.0, v = 0.0, w = 0.0;   // weights of a, b, c
    const double d1 = (ab[0] * ap[0] + ab[1] * ap[1]) + ab[2] * ap[2];
    const double d2 = (ac[0] * ap[0] + ac[1] * ap[1]) + ac[2] * ap[2];
    const double d3 = (ab[0] * bp[0] + ab[1] * bp[1]) + ab[2] * bp[2];
    const double d4 = (ac[0] * bp[0] + ac[1] * bp[1]) + ac[2] * bp[2];
    const double d5 = (ab[0] * cq[0] + ab[1] * cq[1]) + ab[2] * cq[2];
    const double d6 = (ac[0] * cq[0] + ac[1] * cq[1]) + ac[2] * cq[2];
    const double vc = d1 * d4 - d3 * d2;
    const double vb = d5 * d2 - d1 * d6;
    const double va = d3 * d6 - d5 * d4;
    int region;
    if (d1 <= 0.0 && d2 <= 0.0) region = 0;                                  // vertex a
    else if (d3 >= 0.0 && d4 <= d3) region = 1;                              // vertex b
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) region = 2;                // edge ab
    else if (d6 >= 0.0 && d5 <= d6) region = 3;                              // vertex c
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) region = 4;                // edge ac
    else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) region = 5;  // edge bc
    else region = 6;                                                         // face
    switch (region) {
    case 0: break;
    case 1: u = 0.0; v = 1.0; break;
    case 2: v = ratio(d1, d1 - d3); u = 1.0 - v; break;
    case 3: u = 0.0; w = 1.0; break;
    case 4: w = ratio(d2, d2 - d6); u = 1.0 - w; break;
    case 5: { const double e = d4 - d3; w = ratio(e, e + (d5 - d6)); u = 0.0; v = 1.0 - w; break; }
    default: {
        const double s = (va + vb) + vc;
        if (!(va >= 0.0 && vb >= 0.0 && vc >= 0.0 && s > 0.0)) return closest_on_edges(p, a, b, c);
        v = vb / s; w = vc / s; u = (1.0 - v) - w;
    }
    }
    // the point: a vertex exactly, b + w (c - b) on bc, a + v ab + w ac otherwise
    double r[3];
    for (int k = 0; k < 3; k++) {
        double q;
        if (region == 0) q = a[k];
        else if (region == 1) q = b[k];
        else if (region == 3) q = c[k];
        else if (region == 5) q = b[k] + (c[k] - b[k]) * w;
        else q = (a[k] + ab[k] * v) + ac[k] * w;
        R.cp[k] = q;
        r[k] = p[k] - q;
    }
    R.d2 = sq3(r);
    R.w[0] = u; R.w[1] = v; R.w[2] = w;
    return R;
}

// ---- exact orientation in the xy plane ------------------------------------------------------------------------------------
// TwoSum (Knuth): s + e == a + b exactly (binary64, no overflow)
SDFK_TRI_HD inline void two_sum(double a, double b, double* s, double* e)
{
    const double x = a + b;
    const double bv = x - a;
    const double av = x - bv;
    *s = x;
    *e = (a - av) + (b - bv);
}

// The exact sign of t[0] + ... + t[n-1] (n <= 6): Shewchuk's Grow-Expansion turns the terms into a nonoverlapping expansion,
// whose sign is the sign of its largest nonzero component.
SDFK_TRI_HD inline int exact_sign_sum(const double* t, int n)
{
    double e[6];
    int m = 0;
    for (int i = 0; i < n; i++) {
        double q = t[i];
        for (int j = 0; j < m; j++) {
            double s, err;
            two_sum(q, e[j], &s, &err);
            e[j] = err;
            q = s;
        }
        e[m++] = q;
    }
    for (int j = m - 1; j >= 0; j--)
        if (e[j] != 0.0) return e[j] > 0.0 ? 1 : -1;
    return 0;
}

// sign of (bx - ax) (py - ay) - (by - ay) (px - ax), exactly: expanded into six products of two binary32 values, each exact in
// binary64 (the ax ay terms cancel).
SDFK_TRI_HD inline int orient2d_exact(float ax, float ay, float bx, float by, float px, float py)
{
    const double t[6] = {(double)bx * (double)py, -((double)bx * (double)ay), -((double)ax * (double)py),
                         -((double)by * (double)px), (double)by * (double)ax, (double)ay * (double)px};
    return exact_sign_sum(t, 6);
}

// The orientation of (a, b) and the column point moved by (+eps, +eps^2): the exact sign when it is not zero, else the sign of
// -(by - ay) (the eps term), else of (bx - ax) (the eps^2 term).  Zero only when a == b.
SDFK_TRI_HD inline int orient2d_perturbed(float ax, float ay, float bx, float by, float px, float py)
{
    const int s = orient2d_exact(ax, ay, bx, by, px, py);
    if (s) return s;
    if (by != ay) return by < ay ? 1 : -1;
    if (bx != ax) return bx > ax ? 1 : -1;
    return 0;
}

// The sign of the projected area of (a, b, c): orient2d of (a, b) and c.  0: the triangle covers no column.
SDFK_TRI_HD inline int projected_area_sign(const float a[3], const float b[3], const float c[3])
{
    return orient2d_exact(a[0], a[1], b[0], b[1], c[0], c[1]);
}

// Does the column (px, py), perturbed, lie inside the projection of (a, b, c), whose exact area sign is `area` (nonzero)?
// Every edge must see the point on the side of the third vertex.
SDFK_TRI_HD inline bool column_inside(const float a[3], const float b[3], const float c[3], int area, float px, float py)
{
    return orient2d_perturbed(a[0], a[1], b[0], b[1], px, py) == area && orient2d_perturbed(b[0], b[1], c[0], c[1], px, py) == area &&
           orient2d_perturbed(c[0], c[1], a[0], a[1], px, py) == area;
}

// The z at which column (px, py) crosses the plane of (a, b, c): barycentric weights from the binary64 edge functions, turned
// to the area's sign and clamped at 0, then (wa az + wb bz) + wc cz over their sum; az if the sum is not positive.  A convex
// combination of the vertex z, so never NaN.
SDFK_TRI_HD inline double edge_f64(const float a[3], const float b[3], double px, double py)
{
    return ((double)b[0] - (double)a[0]) * (py - (double)a[1]) - ((double)b[1] - (double)a[1]) * (px - (double)a[0]);
}

SDFK_TRI_HD inline double z_cross(const float a[3], const float b[3], const float c[3], int area, float px, float py)
{
    const double x = px, y = py, sg = area > 0 ? 1.0 : -1.0;
    double wa = edge_f64(b, c, x, y) * sg, wb = edge_f64(c, a, x, y) * sg, wc = edge_f64(a, b, x, y) * sg;
    wa = wa > 0.0 ? wa : 0.0;
    wb = wb > 0.0 ? wb : 0.0;
    wc = wc > 0.0 ? wc : 0.0;
    const double s = (wa + wb) + wc;
    if (!(s > 0.0)) return (double)a[2];
    return (((wa * (double)a[2]) + (wb * (double)b[2])) + (wc * (double)c[2])) / s;
}

// ---- the columns of a volume ----------------------------------------------------------------------------------------------
// column / plane i of an axis that starts at m with spacing d (f32, as the volume's cell centres are computed)
SDFK_TRI_HD inline float col_coord(float m, int i, float d) { return m + (float)i * d; }

// The columns i whose coordinate lies in [lo, hi]: [*i0, *i1] (empty when *i0 > *i1).  An estimate, then exact steps along the
// monotone coordinate sequence.  A spacing that is not positive and finite gives the whole range [0, n - 1].
SDFK_TRI_HD inline void col_range(float lo, float hi, float m, float d, int n, int* i0, int* i1)
{
    if (!(d > 0.0f) || !std::isfinite(d)) { *i0 = 0; *i1 = n - 1; return; }
    double e0 = std::floor(((double)lo - (double)m) / (double)d), e1 = std::ceil(((double)hi - (double)m) / (double)d);
    int a = (int)std::fmin(std::fmax(e0, 0.0), (double)n), b = (int)std::fmin(std::fmax(e1, -1.0), (double)(n - 1));
    while (a > 0 && col_coord(m, a - 1, d) >= lo) a--;
    while (a < n && col_coord(m, a, d) < lo) a++;
    while (b < n - 1 && col_coord(m, b + 1, d) <= hi) b++;
    while (b >= 0 && col_coord(m, b, d) > hi) b--;
    *i0 = a;
    *i1 = b;
}

// The f32 colour blend: weights rounded to f32, (ca wa + cb wb) + cc wc per channel.
SDFK_TRI_HD inline void blend_colour(const float ca[3], const float cb[3], const float cc[3], const double w[3], float out[3])
{
    const float wa = (float)w[0], wb = (float)w[1], wc = (float)w[2];
    for (int k = 0; k < 3; k++) out[k] = (ca[k] * wa + cb[k] * wb) + cc[k] * wc;
}

}  // namespace sdfk_trimesh_sdf
