// trimesh_simplify.h -- the decisions and the arithmetic of sdfk_trimesh_simplify (lib_trimesh_simplify.hip: vertex clustering, the
// vertices of a triangle mesh grouped by the cell of a lattice as sdfk_trimesh_weld groups them, every group replaced by ONE MADE
// vertex, the triangles that fall on top of each other cleaned up): which arguments are accepted, the position and colour of a
// group under the three placements, the records of the triangle sorts, which triangle of a run of equal vertex sets is kept.
// Plain C++ outside hipcc, so that tests/cpp/mesh_simplify_host.cpp runs exactly the code the kernels run;
// tests/mesh_simplify_model.py restates it in numpy.  Contract: include/sdfkit_hip.h, "Triangle meshes: simplification".
//
// Every decision is made on integers.  The arithmetic is binary64 from the f32 inputs, one rounding per written operation, in the
// order written (-ffp-contract=off), + - * / and sqrt only, and one final rounding to f32 per output component.  The grouping
// itself (lattice_of, lattice_key, the pass masks, heads and representatives) is trimesh_weld.h's; the chunked sum is
// points_filter.h's (Sum3, kChunk); the eigen-solve is points_normals.h's (Eigen3).
#pragma once
#include <cstdint>

#include "points_normals.h"   // Cov, Eigen3
#include "trimesh_weld.h"     // the lattice, index_degenerate; with it points_filter.h and trimesh_topology.h

namespace sdfk_trimesh_simp {

using sdfk_filter::kChunk;
using sdfk_filter::Sum3;
using sdfk_trimesh_topo::index_bytes;
using sdfk_trimesh_topo::index_degenerate;

enum { kRepresentative = 0, kCentroid = 1, kQuadric = 2 };                     // SDFK_SIMPLIFY_*: the placements
enum { kKeepDuplicates = 1, kCancelPairs = 2, kKnownFlags = 3 };               // SDFK_SIMPLIFY_*: the flags
enum { kStatMerged = 0, kStatDegenerate, kStatDuplicates, kStatUnreferenced, kStatPasses, kStatFallbacks, kStats };
constexpr double kTruncation = 1e-3;   // an eigenpair takes part in the minimiser iff l_i > kTruncation * l_max

// ---- what is accepted -----------------------------------------------------------------------------------------------------------
SDFK_TRI_HD inline bool cell_is_valid(float cell) { return cell > 0.0f && cell < INFINITY; }   // (false for NaN)
SDFK_TRI_HD inline bool placement_is_valid(int32_t placement) { return placement >= kRepresentative && placement <= kQuadric; }
SDFK_TRI_HD inline bool flags_are_known(int32_t flags) { return (flags & ~kKnownFlags) == 0; }
SDFK_TRI_HD inline bool flags_are_compatible(int32_t flags) { return (flags & kKnownFlags) != kKnownFlags; }   // keep them all AND cancel pairs: refused

// ---- the centroid -----------------------------------------------------------------------------------------------------------------
// member(i), i = 0 .. count - 1: the vertices of the group in ascending index.  The mean of the rows a3[3 member(i)] per axis: the
// members are cut into chunks of kChunk in that order (the last may be short); a chunk is a Sum3 that takes its members in order
// (each widened first), the total a Sum3 that takes the chunk sums in order, both from +0.0; mean = total / (double)count, once.
template <class M>
SDFK_TRI_HD inline void chunked_mean(const float* a3, M member, int64_t count, double mean[3])
{
    Sum3 total;
    for (int64_t i = 0; i < count; i += kChunk) {
        Sum3 chunk;
        const int64_t end = i + kChunk < count ? i + kChunk : count;
        for (int64_t j = i; j < end; j++) {
            const float* p = a3 + 3 * (int64_t)member(j);
            chunk.add_point(p[0], p[1], p[2]);
        }
        total.add_sum(chunk.v);
    }
    for (int a = 0; a < 3; a++) mean[a] = total.v[a] / (double)count;
}

// ---- the quadric ------------------------------------------------------------------------------------------------------------------
// a: the entries 00, 01, 02, 11, 12, 22 of the sum of n n^T; b: the sum of d n.  All from +0.0.
struct Quadric {
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double b[3] = {0.0, 0.0, 0.0};
    // One triangle (p0, p1, p2), c the group's centroid before its rounding: q_k = (double)p_k - c per component;
    // e1 = q1 - q0, e2 = q2 - q0; n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x) -- not normalised, so the weight
    // of a triangle is its area squared; d = -((n0 q0x + n1 q0y) + n2 q0z).  Then a00 += n0 n0, a01 += n0 n1, a02 += n0 n2,
    // a11 += n1 n1, a12 += n1 n2, a22 += n2 n2, b0 += d n0, b1 += d n1, b2 += d n2.
    SDFK_TRI_HD void add_triangle(const float* p0, const float* p1, const float* p2, const double c[3])
    {
        double q0[3], e1[3], e2[3];
        for (int k = 0; k < 3; k++) {
            q0[k] = (double)p0[k] - c[k];
            const double q1 = (double)p1[k] - c[k], q2 = (double)p2[k] - c[k];
            e1[k] = q1 - q0[k];
            e2[k] = q2 - q0[k];
        }
        const double n0 = e1[1] * e2[2] - e1[2] * e2[1];
        const double n1 = e1[2] * e2[0] - e1[0] * e2[2];
        const double n2 = e1[0] * e2[1] - e1[1] * e2[0];
        const double d = -((n0 * q0[0] + n1 * q0[1]) + n2 * q0[2]);
        a[0] = a[0] + n0 * n0; a[1] = a[1] + n0 * n1; a[2] = a[2] + n0 * n2;
        a[3] = a[3] + n1 * n1; a[4] = a[4] + n1 * n2; a[5] = a[5] + n2 * n2;
        b[0] = b[0] + d * n0; b[1] = b[1] + d * n1; b[2] = b[2] + d * n2;
    }
    SDFK_TRI_HD void add(const Quadric& q)
    {
        for (int k = 0; k < 6; k++) a[k] = a[k] + q.a[k];
        for (int k = 0; k < 3; k++) b[k] = b[k] + q.b[k];
    }
};

// The quadric of a group about c.  A member's quadric takes the triangles of its incident corners inc[inc_start[v] ..
// inc_start[v + 1]) in that (ascending) order -- the adjacency lists no corner of an index-degenerate triangle -- each triangle's
// positions gathered through idx.  A chunk's quadric takes its members' in order, the total the chunks' in order: the chunking of
// the centroid.  A TRIANGLE WITH TWO CORNERS IN THE GROUP COUNTS TWICE (with three, three times): it is reached from each.
template <class M>
SDFK_TRI_HD inline Quadric group_quadric(const float* pos, const int32_t* idx, const uint32_t* inc_start, const uint32_t* inc, M member, int64_t count,
                                         const double c[3])
{
    Quadric total;
    for (int64_t i = 0; i < count; i += kChunk) {
        Quadric chunk;
        const int64_t end = i + kChunk < count ? i + kChunk : count;
        for (int64_t j = i; j < end; j++) {
            const int64_t v = (int64_t)member(j);
            Quadric own;
            for (uint32_t e = inc_start[v]; e < inc_start[v + 1]; e++) {
                const int32_t* tri = idx + 3 * (int64_t)(inc[e] / 3u);
                own.add_triangle(pos + 3 * (int64_t)tri[0], pos + 3 * (int64_t)tri[1], pos + 3 * (int64_t)tri[2], c);
            }
            chunk.add(own);
        }
        total.add(chunk);
    }
    return total;
}

// Lindstrom's minimiser of the quadric, relative to c, without a square root of its own and without an order: A is decomposed by
// Eigen3 (its fixed sweeps; eigenvalues l_i = the diagonal, eigenvectors v_i = the columns).  l_max = l_0, replaced by l_1 when
// l_1 > l_max, then by l_2 likewise.  false (no minimiser) when l_max > 0 does not hold.  Otherwise x = (0, 0, 0), and for
// i = 0, 1, 2 in this order, when l_i > kTruncation * l_max:
//   s = (v_0i (-b0) + v_1i (-b1)) + v_2i (-b2);  t = s / l_i;  x_k = x_k + v_ki t  (k = 0, 1, 2).
SDFK_TRI_HD inline bool minimiser(const Quadric& Q, double x[3])
{
    sdfk_pc::Cov C;
    C.c00 = Q.a[0]; C.c01 = Q.a[1]; C.c02 = Q.a[2]; C.c11 = Q.a[3]; C.c12 = Q.a[4]; C.c22 = Q.a[5];
    sdfk_pc::Eigen3 E;
    E.solve(C);
    const double l[3] = {E.a[0][0], E.a[1][1], E.a[2][2]};
    double lmax = l[0];
    if (l[1] > lmax) lmax = l[1];
    if (l[2] > lmax) lmax = l[2];
    x[0] = x[1] = x[2] = 0.0;
    if (!(lmax > 0.0)) return false;
    const double cut = kTruncation * lmax;
    const double nb[3] = {-Q.b[0], -Q.b[1], -Q.b[2]};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 3; i++) {
        if (!(l[i] > cut)) continue;
        const double s = (E.v[0][i] * nb[0] + E.v[1][i] * nb[1]) + E.v[2][i] * nb[2];
        const double t = s / l[i];
        for (int k = 0; k < 3; k++) x[k] = x[k] + E.v[k][i] * t;
    }
    return true;
}

// The cell of the lattice along one axis, k = voxel_of(p, 0, cell) of any member (an integer-valued binary64), is
// [k cell, (k + 1) cell) in binary64; p lies in it iff it is finite and k cell <= p < (k + 1) cell.
SDFK_TRI_HD inline bool in_cell(double p, double k, float cell)
{
    const double lo = k * (double)cell, hi = (k + 1.0) * (double)cell;
    return (p < 0.0 ? -p : p) < (double)INFINITY && p >= lo && p < hi;
}

// ---- one group's vertex ---------------------------------------------------------------------------------------------------------
// -> whether the quadric placement fell back to the centroid.  col: the mesh's colours, or null (then zeros).
//   kRepresentative  the position and colour BITS of member(0), the lowest index: nothing is computed.
//   kCentroid        position = (float)mean of the positions, colour = (float)mean of the colours (chunked_mean of each).
//   kQuadric         c = the mean of the positions before its rounding; p = c + x, x the minimiser of the group's quadric about c;
//                    the centroid instead -- a fallback -- when there is no minimiser or some p_a is not in the group's cell
//                    along axis a (in_cell: a non-finite p_a is in no cell).  Colours as for the centroid.
template <class M>
SDFK_TRI_HD inline bool place_group(int32_t placement, const float* pos, const float* col, const int32_t* idx, const uint32_t* inc_start,
                                    const uint32_t* inc, float cell, M member, int64_t count, float out_pos[3], float out_col[3])
{
    const int64_t first = (int64_t)member(0);
    if (placement == kRepresentative) {
        __builtin_memcpy(out_pos, pos + 3 * first, 3 * sizeof(float));   // (as bits)
        if (col) __builtin_memcpy(out_col, col + 3 * first, 3 * sizeof(float));
        else out_col[0] = out_col[1] = out_col[2] = 0.0f;
        return false;
    }
    double c[3], p[3];
    chunked_mean(pos, member, count, c);
    bool fallback = false;
    if (placement == kQuadric) {
        double x[3];
        bool ok = minimiser(group_quadric(pos, idx, inc_start, inc, member, count, c), x);
        for (int a = 0; a < 3; a++) {
            p[a] = c[a] + x[a];
            ok = ok && in_cell(p[a], sdfk_filter::voxel_of(pos[3 * first + a], 0.0f, cell), cell);
        }
        fallback = !ok;
    }
    for (int a = 0; a < 3; a++) out_pos[a] = (float)(placement == kQuadric && !fallback ? p[a] : c[a]);
    if (col) {
        double m[3];
        chunked_mean(col, member, count, m);
        for (int a = 0; a < 3; a++) out_col[a] = (float)m[a];
    } else {
        out_col[0] = out_col[1] = out_col[2] = 0.0f;
    }
    return fallback;
}

// ---- the triangles --------------------------------------------------------------------------------------------------------------
// Groups are numbered by ascending representative; a triangle's corners as group numbers (ga, gb, gc).  Its vertex set is the
// sorted triple lo < mid < hi, whatever its winding.  An index-degenerate triangle has none: its records carry the triple
// (0, 0, 0), which no vertex set equals, and it is dropped whatever run it lands in.
struct Triple {
    uint32_t lo, mid, hi;
};
SDFK_TRI_HD inline Triple sorted_triple(uint32_t a, uint32_t b, uint32_t c)
{
    if (index_degenerate((int32_t)a, (int32_t)b, (int32_t)c)) return Triple{0u, 0u, 0u};
    const uint32_t lo = a < b ? (a < c ? a : c) : (b < c ? b : c);
    const uint32_t hi = a > b ? (a > c ? a : c) : (b > c ? b : c);
    return Triple{lo, (a ^ b ^ c) ^ lo ^ hi, hi};
}
SDFK_TRI_HD inline bool has_vertex_set(const Triple& t) { return t.hi != 0u; }
// 96 bits for a 64-bit sort key: sorted by lo first, then -- stably -- by (hi above mid): equal sets end adjacent, in ascending
// triangle index.  The passes: the bytes a group number below `groups` can set, in each part.
SDFK_TRI_HD inline uint64_t triple_key_first(const Triple& t) { return (uint64_t)t.lo; }
SDFK_TRI_HD inline uint64_t triple_key_second(const Triple& t) { return (uint64_t)t.hi << 32 | (uint64_t)t.mid; }
SDFK_TRI_HD inline unsigned triple_mask_first(int64_t groups) { return (1u << index_bytes(groups)) - 1u; }
SDFK_TRI_HD inline unsigned triple_mask_second(int64_t groups) { return sdfk_trimesh_topo::key_digit_mask(groups); }
SDFK_TRI_HD inline bool same_set(uint64_t second, uint32_t lo, uint64_t prev_second, uint32_t prev_lo) { return second == prev_second && lo == prev_lo; }
// first: the record is the first of its run of equal sets (the lowest triangle index of the set); run: the length of that run.
//   default          the first of every run is kept, with its own winding;
//   kCancelPairs     the first of a run of odd length is kept, a run of even length is dropped entirely.
// (kKeepDuplicates sorts nothing: every triangle that is not index-degenerate is kept.)
SDFK_TRI_HD inline bool keeps_in_run(bool set, bool first, uint32_t run, int32_t flags)
{
    return set && first && (!(flags & kCancelPairs) || (run & 1u) != 0u);
}
SDFK_TRI_HD inline int triangle_passes(int64_t groups, int32_t flags) { return (flags & kKeepDuplicates) ? 0 : 3 * index_bytes(groups); }

// A group is kept iff some kept triangle names it.
SDFK_TRI_HD inline bool keeps_group(int32_t v, int32_t rep_v, bool used) { return rep_v == v && used; }

}  // namespace sdfk_trimesh_simp
