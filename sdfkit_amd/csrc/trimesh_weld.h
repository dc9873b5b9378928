// trimesh_weld.h -- the decisions of sdfk_trimesh_weld (lib_trimesh_weld.hip: the vertices of a triangle mesh grouped by position,
// every group replaced by its lowest index): the group key of a vertex in both modes, the passes a sort needs, what a sorted
// record starts, which triangles and vertices are kept, and what the map says.  Plain C++ outside hipcc, so that
// tests/cpp/mesh_weld_host.cpp runs exactly the code the kernels run.  Every decision is made on integers (the bits of the
// coordinates, or the lattice cell that points_filter.h computes in binary64): nothing here depends on an order.
#pragma once
#include <cstdint>

#include "points_filter.h"      // voxel_of, voxel_key, span_is_valid, span_bits, digit_mask: the lattice of the voxel filter
#include "trimesh_topology.h"   // index_degenerate

namespace sdfk_trimesh_wld {

using sdfk_filter::Lattice;
using sdfk_trimesh_topo::index_degenerate;

enum { kKeepDegenerate = 1, kKeepUnreferenced = 2, kKnownFlags = 3 };   // SDFK_WELD_*
enum { kStatMerged = 0, kStatDegenerate, kStatUnreferenced, kStatPasses };

SDFK_TRI_HD inline float float_of(uint32_t u)
{
    float f;
    __builtin_memcpy(&f, &u, sizeof f);
    return f;
}

// ---- exact mode: the 96 bits of a position, -0 mapped to +0 ---------------------------------------------------------------------
// The handle holds no NaN and no infinity, so two coordinates are equal as values iff their canonical bits are equal (a
// subnormal is its own value: nothing is flushed, no arithmetic is done).
SDFK_TRI_HD inline uint32_t canon_bits(uint32_t b) { return b == 0x80000000u ? 0u : b; }
// The key of the first sort (x) and of the second (z above y): the records end in (z, y, x) order, which nobody relies on --
// only that equal positions are adjacent and, the sorts being stable from ascending indices, ascending in index.
SDFK_TRI_HD inline uint64_t exact_key_first(const uint32_t p[3]) { return (uint64_t)canon_bits(p[0]); }
SDFK_TRI_HD inline uint64_t exact_key_second(const uint32_t p[3]) { return (uint64_t)canon_bits(p[2]) << 32 | (uint64_t)canon_bits(p[1]); }
SDFK_TRI_HD inline bool exact_same(const uint32_t p[3], const uint32_t q[3])
{
    return canon_bits(p[0]) == canon_bits(q[0]) && canon_bits(p[1]) == canon_bits(q[1]) && canon_bits(p[2]) == canon_bits(q[2]);
}

// ---- lattice mode: the cell of a world-anchored lattice, origin (0, 0, 0) -------------------------------------------------------
SDFK_TRI_HD inline bool tolerance_is_valid(float tol) { return tol >= 0.0f && tol < INFINITY; }   // (false for NaN)
SDFK_TRI_HD inline uint64_t lattice_key(const Lattice& L, const uint32_t p[3]) { return sdfk_filter::voxel_key(L, float_of(p[0]), float_of(p[1]), float_of(p[2])); }

// The bits of a float as an unsigned integer that orders as the value does (-0 just below +0): the per-axis minimum and maximum
// over all vertices are integer atomicMin / atomicMax of these.  voxel_of is monotone, so the least cell is the cell of the
// least coordinate.
SDFK_TRI_HD inline uint32_t ordered_bits(uint32_t b) { return (b & 0x80000000u) ? ~b : b | 0x80000000u; }
SDFK_TRI_HD inline uint32_t unordered_bits(uint32_t o) { return (o & 0x80000000u) ? o & 0x7fffffffu : ~o; }

// The lattice of a tolerance over the box [lo, hi] of all vertices and the passes its key can need; false: an axis spans 2^21
// cells or more.
inline bool lattice_of(float tol, const float lo[3], const float hi[3], Lattice* L, unsigned* mask)
{
    int bits[3];
    L->size = tol;
    for (int a = 0; a < 3; a++) {
        L->origin[a] = 0.0f;
        const double kmin = sdfk_filter::voxel_of(lo[a], 0.0f, tol), kmax = sdfk_filter::voxel_of(hi[a], 0.0f, tol);
        if (!sdfk_filter::span_is_valid(kmin, kmax)) return false;
        L->kmin[a] = kmin;
        bits[a] = sdfk_filter::span_bits(kmin, kmax);
    }
    *mask = sdfk_filter::digit_mask(bits);
    return true;
}

// ---- pass skipping --------------------------------------------------------------------------------------------------------------
// diff: the OR over all records of key ^ key[0].  Byte d of it is zero iff all keys agree in byte d, and a pass over such a byte
// moves nothing (the sort is stable): it is not run.
SDFK_TRI_HD inline uint64_t key_diff(uint64_t key, uint64_t key0) { return key ^ key0; }
SDFK_TRI_HD inline unsigned pass_mask(uint64_t diff)
{
    unsigned m = 0;
    for (int d = 0; d < 8; d++)
        if (diff >> (8 * d) & 255u) m |= 1u << d;
    return m;
}
SDFK_TRI_HD inline int passes_of(unsigned mask)
{
    int n = 0;
    for (int d = 0; d < 8; d++) n += (int)(mask >> d & 1u);
    return n;
}

// ---- groups ---------------------------------------------------------------------------------------------------------------------
// A sorted record is the head of its group iff it is the first or its key differs from its predecessor's (exact mode: `same` is
// exact_same of the two positions, gathered through the records' indices; lattice mode: the equality of the two keys).
SDFK_TRI_HD inline bool is_head(int64_t j, bool same_as_predecessor) { return j == 0 || !same_as_predecessor; }
// scanned: the exclusive count of heads before sorted position j
SDFK_TRI_HD inline uint32_t group_of(uint32_t scanned, bool head) { return head ? scanned : scanned - 1u; }

// ---- what is kept ---------------------------------------------------------------------------------------------------------------
SDFK_TRI_HD inline bool flags_are_valid(int32_t flags) { return (flags & ~kKnownFlags) == 0; }
// (a, b, c): the representatives of the triangle's corners
SDFK_TRI_HD inline bool keeps_triangle(int32_t a, int32_t b, int32_t c, int32_t flags) { return (flags & kKeepDegenerate) != 0 || !index_degenerate(a, b, c); }
// used: some kept triangle names v as a representative
SDFK_TRI_HD inline bool keeps_vertex(int32_t v, int32_t rep_v, bool used, int32_t flags) { return rep_v == v && (used || (flags & kKeepUnreferenced) != 0); }
// vertex_map of a vertex whose representative has the new number n when it is kept
SDFK_TRI_HD inline int32_t map_of(bool rep_kept, uint32_t n) { return rep_kept ? (int32_t)n : -1; }

}  // namespace sdfk_trimesh_wld
