// trimesh_winding.h -- the arithmetic of sdfk_trimesh_winding / sdfk_trimesh_to_volume_signed (lib_trimesh_winding.hip): the
// generalized winding number of a triangle mesh (Jacobson et al. 2013) summed over a hierarchy of clusters (the first-order term
// of Barill et al. 2018).  Contract: include/sdfkit_hip.h, "Triangle meshes: generalized winding number".  Plain C++ outside hipcc
// (no contraction: -ffp-contract=off), binary64 + - * / sqrt rint only, so that a host program runs the very code the kernels run
// (tests/cpp/mesh_winding_host.cpp) and numpy restates it bit for bit (tests/mesh_winding_model.py).
//
// THE HIERARCHY.  L = levels_for(nt): the least L with 16 * 4^L >= nt, at most kMaxLevel.  A lattice of 2^L cells per axis covers
// the cube that starts at the low corner of the mesh's f32 box and has the box's greatest extent as its edge.  A triangle belongs to
// the cell of its centroid ((a + b) + c) / 3 (binary64); the cell's three indices are interleaved into a code m of 3 L bits, x in
// the lowest bit of every triple.  The triangles are sorted by (m, index).  The nodes of level l (0: the root, L: the lattice
// cells) are the dense array of the 8^l codes of 3 l bits; node (l, m) has the number (8^l - 1) / 7 + m, so the children of node n
// are 8 n + 1 + c, c = 0 .. 7 (c = dx + 2 dy + 4 dz), its parent is (n - 1) / 8, and the triangles of every node are one run
// [start, start + count) of the sorted order.  An empty node has count 0.
// Moments.  Per triangle: n = (b - a) x (c - a), weight = |n| (twice the area), centroid as above.  A cell's sums -- of n, of
// weight * centroid, of weight -- start from 0 and add its triangles in sorted order; a node's sums above the cells start from 0 and
// add its eight children's sums, c = 0 .. 7.  Then N = 0.5 * sum n; P = sum(weight * centroid) / sum weight, or, when no triangle
// of the node has an area, the centroid of its first triangle; r2 = the greatest |v - P|^2 over the vertices of its triangles
// (a maximum: order-free).
//
// THE SUM of one finite query q, started from w = 0 at the root, depth first, children in the order c = 0 .. 7; at a node with
// count > 0, with D = P - q and d2 = |D|^2:
//   d2 > beta^2 r2 (beta^2 = beta * beta rounded once; a NaN product -- beta = +inf, r2 = 0 -- compares false):
//                                                   w += (D . N) / (4 pi (d2 sqrt(d2)))                      (a cluster term)
//   else, at level L or with count <= kDirect:       w += atan2(det, den) / (2 pi) for every triangle of the run, in sorted order
//   else:                                            the children.
// w is summed in exactly this order, in binary64: one lane owns one query, so there is no order of lanes or atomics to depend on,
// the order is part of the statement, and no term is rounded to anything coarser on its way.  (A 64-bit fixed point would free the model
// of the order, at the price of a rounding step per term and a range to defend; with one lane per query there is nothing to free.)
// Every dot product and squared length is (x0 y0 + x1 y1) + x2 y2.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SDFK_WN_HD __host__ __device__ __forceinline__
#else
#define SDFK_WN_HD inline
#endif

namespace sdfk_trimesh_wn {

constexpr int kMaxLevel = 6;         // 64 cells per axis; 299593 nodes
constexpr uint32_t kDirect = 4;      // an opened node with this many triangles or fewer adds them itself
constexpr double kPi = 0x1.921fb54442d18p+1, kTwoPi = 0x1.921fb54442d18p+2, kFourPi = 0x1.921fb54442d18p+3;

SDFK_WN_HD int levels_for(int64_t nt)
{
    int L = 0;
    while (L < kMaxLevel && (int64_t(16) << (2 * L)) < nt) L++;
    return L;
}
SDFK_WN_HD uint32_t level_offset(int l) { return (uint32_t)(((uint64_t(1) << (3 * l)) - 1) / 7); }
SDFK_WN_HD uint32_t node_total(int L) { return level_offset(L + 1); }

struct Lattice {
    double lo[3];
    double scale;   // cells per unit length; 0 when the box is a point
    int L;
};

SDFK_WN_HD Lattice lattice_for(const float lo[3], const float hi[3], int64_t nt)
{
    Lattice A;
    A.L = levels_for(nt);
    double ext = 0.0;
    for (int a = 0; a < 3; a++) {
        A.lo[a] = (double)lo[a];
        const double e = (double)hi[a] - (double)lo[a];
        if (e > ext) ext = e;
    }
    A.scale = ext > 0.0 ? (double)(1 << A.L) / ext : 0.0;
    return A;
}

SDFK_WN_HD double dot3(const double x[3], const double y[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

SDFK_WN_HD void tri_centroid(const float a[3], const float b[3], const float c[3], double ctr[3])
{
    for (int k = 0; k < 3; k++) ctr[k] = (((double)a[k] + (double)b[k]) + (double)c[k]) / 3.0;
}

// the code of the centroid's cell: per axis (int)((ctr - lo) * scale), clamped to [0, 2^L - 1]
SDFK_WN_HD uint32_t leaf_code(const Lattice& A, const double ctr[3])
{
    const int n = 1 << A.L;
    uint32_t m = 0;
    for (int a = 0; a < 3; a++) {
        const double u = (ctr[a] - A.lo[a]) * A.scale;
        const int k = u >= (double)n ? n - 1 : (u > 0.0 ? (int)u : 0);
        for (int b = 0; b < A.L; b++) m |= (uint32_t)((k >> b) & 1) << (3 * b + a);
    }
    return m;
}

struct Sums {
    double n[3], wc[3], w;
};

SDFK_WN_HD Sums no_sums()
{
    Sums S;
    for (int k = 0; k < 3; k++) S.n[k] = S.wc[k] = 0.0;
    S.w = 0.0;
    return S;
}

SDFK_WN_HD void add_triangle(Sums& S, const float a[3], const float b[3], const float c[3])
{
    double e1[3], e2[3], n[3], ctr[3];
    for (int k = 0; k < 3; k++) {
        e1[k] = (double)b[k] - (double)a[k];
        e2[k] = (double)c[k] - (double)a[k];
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double w = __builtin_sqrt(dot3(n, n));
    tri_centroid(a, b, c, ctr);
    for (int k = 0; k < 3; k++) {
        S.n[k] = S.n[k] + n[k];
        S.wc[k] = S.wc[k] + w * ctr[k];
    }
    S.w = S.w + w;
}

SDFK_WN_HD void add_sums(Sums& S, const Sums& C)
{
    for (int k = 0; k < 3; k++) {
        S.n[k] = S.n[k] + C.n[k];
        S.wc[k] = S.wc[k] + C.wc[k];
    }
    S.w = S.w + C.w;
}

struct Node {
    double N[3], P[3], r2;
    uint32_t start, count;
};

// N and P of a node from its sums; first_ctr: the centroid of the first triangle of its run
SDFK_WN_HD void node_moments(const Sums& S, const double first_ctr[3], double N[3], double P[3])
{
    for (int k = 0; k < 3; k++) {
        N[k] = 0.5 * S.n[k];
        P[k] = S.w > 0.0 ? S.wc[k] / S.w : first_ctr[k];
    }
}

SDFK_WN_HD double vertex_r2(const float v[3], const double P[3])
{
    const double e[3] = {(double)v[0] - P[0], (double)v[1] - P[1], (double)v[2] - P[2]};
    return dot3(e, e);
}

SDFK_WN_HD double atan_eighth(int j)   // atan(j / 8) rounded to binary64 (mathops.h's table)
{
    switch (j) {
    case 0: return 0.0;
    case 1: return 0x1.fd5ba9aac2f6ep-4;
    case 2: return 0x1.f5b75f92c80ddp-3;
    case 3: return 0x1.6f61941e4def1p-2;
    case 4: return 0x1.dac670561bb4fp-2;
    case 5: return 0x1.1e00babdefeb4p-1;
    case 6: return 0x1.4978fa3269ee1p-1;
    case 7: return 0x1.700a7c5784634p-1;
    default: return 0x1.921fb54442d18p-1;
    }
}

SDFK_WN_HD bool negative64(double x) { return (__builtin_bit_cast(unsigned long long, x) >> 63) != 0; }

// atan2(y, x) in binary64: mathops.h's scheme without its final rounding to f32.  C99 Annex F for zeros, infinities and NaN;
// otherwise with t = min(|y|, |x|) / max(|y|, |x|): j = rint(8 t), u = (8 t - j) / (8 + t j), atan(t) = atan(j/8) + (u + (u u^2) P(u^2)),
// P = Taylor to u^15; then pi/2 - . when |y| > |x|, pi - . when x < 0, negated when y < 0.
SDFK_WN_HD double atan2_64(double y, double x)
{
    if (x != x || y != y) return x + y;
    const bool xneg = negative64(x);
    if (y == 0.0) return xneg ? (negative64(y) ? -kPi : kPi) : y;
    const double ay = __builtin_fabs(y), ax = __builtin_fabs(x);
    double a;
    if (ax == __builtin_inf() && ay == __builtin_inf()) a = x > 0.0 ? 0x1.921fb54442d18p-1 : 0x1.2d97c7f3321d2p+1;
    else {
        const bool swap = ay > ax;
        const double t = swap ? ax / ay : ay / ax;
        const double j = __builtin_rint(t * 8.0);
        const double u = (t * 8.0 - j) / (8.0 + t * j);
        const double u2 = u * u;
        const double p = -0x1.5555555555555p-2 + u2 * (0x1.999999999999ap-3 + u2 * (-0x1.2492492492492p-3 + u2 * (0x1.c71c71c71c71cp-4
                       + u2 * (-0x1.745d1745d1746p-4 + u2 * (0x1.3b13b13b13b14p-4 + u2 * -0x1.1111111111111p-4)))));
        a = atan_eighth((int)j) + (u + (u * u2) * p);
        if (swap) a = 0x1.921fb54442d18p+0 - a;
        if (x < 0.0) a = kPi - a;
    }
    return y < 0.0 ? -a : a;
}

// Omega / (4 pi) of one triangle (Van Oosterom and Strackee): A = a - q, B = b - q, C = c - q,
//   det = A . (B x C),   den = (((|A| |B|) |C| + (A . B) |C|) + (B . C) |A|) + (C . A) |B|,   term = atan2(det, den) / (2 pi).
// q equal to a vertex: det = +-0 and den = +0, the term is +-0.  q in the triangle's plane: outside the triangle den > 0 and the
// term is det's rounding noise over den, about 0; inside it (and on its edges) den <= 0 and the term is +1/2 or -1/2, by the sign of
// det, which there is rounding noise or a zero.  A triangle with two equal vertices has det = +-0 exactly: its term is +-0 wherever
// den > 0, everywhere off its segment; on the segment den is zero up to rounding, and the term is +-0 or +-1/2 by that rounding.
// Three distinct collinear vertices behave as a triangle seen in its plane.
SDFK_WN_HD double triangle_term(const float a[3], const float b[3], const float c[3], const double q[3])
{
    double A[3], B[3], C[3], x[3];
    for (int k = 0; k < 3; k++) {
        A[k] = (double)a[k] - q[k];
        B[k] = (double)b[k] - q[k];
        C[k] = (double)c[k] - q[k];
    }
    const double la = __builtin_sqrt(dot3(A, A)), lb = __builtin_sqrt(dot3(B, B)), lc = __builtin_sqrt(dot3(C, C));
    x[0] = B[1] * C[2] - B[2] * C[1];
    x[1] = B[2] * C[0] - B[0] * C[2];
    x[2] = B[0] * C[1] - B[1] * C[0];
    const double det = dot3(A, x);
    const double den = (((la * lb) * lc + dot3(A, B) * lc) + dot3(B, C) * la) + dot3(C, A) * lb;
    return atan2_64(det, den) / kTwoPi;
}

SDFK_WN_HD double cluster_term(const double N[3], const double D[3], double d2) { return dot3(D, N) / (kFourPi * (d2 * __builtin_sqrt(d2))); }

SDFK_WN_HD bool finite32(float x) { return __builtin_fabsf(x) <= FLT_MAX; }   // (false for NaN)

struct Counts {
    unsigned long long clusters, triangles;
};

// w of the query q (NaN when a coordinate is NaN or infinite: nothing is visited).  Tris: corners(t, a, b, c) of triangle t.
// The walk keeps no stack: in the numbering above the next node after a finished subtree is found from the node's number alone.
template <class Tris>
SDFK_WN_HD double winding(const Node* nodes, const uint32_t* order, const Tris& T, int L, const float qf[3], double beta2, Counts& K)
{
    if (!(finite32(qf[0]) && finite32(qf[1]) && finite32(qf[2]))) return __builtin_nan("");
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    double w = 0.0;
    uint32_t n = 0;
    int level = 0;
    for (;;) {
        const uint32_t count = nodes[n].count;
        bool down = false;
        if (count) {
            const Node& nd = nodes[n];
            const double D[3] = {nd.P[0] - q[0], nd.P[1] - q[1], nd.P[2] - q[2]};
            const double d2 = dot3(D, D);
            if (d2 > beta2 * nd.r2) {
                w = w + cluster_term(nd.N, D, d2);
                K.clusters++;
            } else if (level == L || count <= kDirect) {
                const uint32_t j0 = nd.start;
                for (uint32_t j = j0; j < j0 + count; j++) {
                    float a[3], b[3], c[3];
                    T.corners(order[j], a, b, c);
                    w = w + triangle_term(a, b, c, q);
                }
                K.triangles += count;
            } else
                down = true;
        }
        if (down) {
            n = 8 * n + 1;
            level++;
            continue;
        }
        while (n && ((n - 1) & 7u) == 7u) {
            n = (n - 1) >> 3;
            level--;
        }
        if (!n) break;
        n++;
    }
    return w;
}

SDFK_WN_HD bool inside_of(double w) { return __builtin_fabs(w) > 0.5; }                        // (false for NaN)
SDFK_WN_HD float winding_f32(double w) { return w != w ? __builtin_nanf("") : (float)w; }

}  // namespace sdfk_trimesh_wn
