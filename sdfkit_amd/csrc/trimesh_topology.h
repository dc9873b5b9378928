// trimesh_topology.h -- the decisions of sdfk_trimesh_components / _topology / _select (lib_trimesh_topology.hip: the connectivity
// of a triangle mesh by index): which triangles connect anything, the key and direction of an edge, the class of an edge from
// its use counts, the steps of the label rounds, the order of the components, the keep rule, and the quantities the host derives
// from a row.  Plain C++ outside hipcc, so that tests/cpp/mesh_topology_host.cpp runs exactly the code the kernels run.  Every
// quantity is an integer: nothing here depends on an order.
#pragma once
#include <cstdint>

#include "trimesh_sdf.h"   // SDFK_TRI_HD

namespace sdfk_trimesh_topo {

// the columns of a component row, and of the mesh census
enum { kTriangles = 0, kVertices, kEdges, kBoundary, kNonManifold, kOdd, kInconsistent, kAreaWeight, kRow };
enum { kCensusComponents = 0, kCensusVertices, kCensusEdges, kCensusBoundary, kCensusNonManifold, kCensusOdd, kCensusInconsistent, kCensusDegenerate };

// A triangle with a repeated index connects nothing, contributes no edge and belongs to no component.
SDFK_TRI_HD inline bool index_degenerate(int32_t a, int32_t b, int32_t c) { return a == b || b == c || a == c; }

// The undirected key of the directed edge (u, v), u != v: min << 32 | max.  Never 0: the key 0 marks a record to skip.
SDFK_TRI_HD inline uint64_t edge_key(int32_t u, int32_t v)
{
    const uint32_t lo = (uint32_t)(u < v ? u : v), hi = (uint32_t)(u < v ? v : u);
    return (uint64_t)lo << 32 | (uint64_t)hi;
}
SDFK_TRI_HD inline bool edge_forward(int32_t u, int32_t v) { return u < v; }
SDFK_TRI_HD inline int32_t edge_low_vertex(uint64_t key) { return (int32_t)(key >> 32); }   // (its component is the edge's)
constexpr uint64_t kSkipKey = 0;

// directed edge k (0, 1, 2) of the triangle (a, b, c): (a, b), (b, c), (c, a)
SDFK_TRI_HD inline void directed_edge(const int32_t tri[3], int k, int32_t* u, int32_t* v)
{
    *u = tri[k];
    *v = tri[k == 2 ? 0 : k + 1];
}

// The class bits of an undirected edge used m >= 1 times, f of them forward.
enum { kIsBoundary = 1, kIsNonManifold = 2, kIsOdd = 4, kIsInconsistent = 8 };
SDFK_TRI_HD inline unsigned edge_class(uint32_t m, uint32_t f)
{
    return (m == 1 ? kIsBoundary : 0u) | (m >= 3 ? kIsNonManifold : 0u) | ((m & 1u) ? kIsOdd : 0u) | ((m == 2 && f != 1) ? kIsInconsistent : 0u);
}

// One edge's contribution to the five edge columns, packed a byte each (edges, boundary, non-manifold, odd, inconsistent): the
// sum over the 64 lanes of a wave cannot carry from one byte into the next.
SDFK_TRI_HD inline uint64_t edge_packed(unsigned cls)
{
    return 1ull | (uint64_t)(cls & kIsBoundary ? 1 : 0) << 8 | (uint64_t)(cls & kIsNonManifold ? 1 : 0) << 16 | (uint64_t)(cls & kIsOdd ? 1 : 0) << 24 |
           (uint64_t)(cls & kIsInconsistent ? 1 : 0) << 32;
}
SDFK_TRI_HD inline uint64_t packed_byte(uint64_t packed, int k) { return packed >> (8 * k) & 255u; }

// The bytes of a vertex index a mesh of nv vertices can set (0 .. 4), and the passes of the sort of the edge keys: those bytes
// of each half of the key.
SDFK_TRI_HD inline int index_bytes(int64_t nv)
{
    int n = 0;
    for (uint64_t top = nv > 0 ? (uint64_t)(nv - 1) : 0; top; top >>= 8) n++;
    return n;
}
SDFK_TRI_HD inline unsigned key_digit_mask(int64_t nv) { return ((1u << index_bytes(nv)) - 1u) * 0x11u; }

// ---- the label rounds: parent[v] <= v always, and parent[v] names a vertex of v's component ---------------------------------
// hook: the least parent of a triangle's corners, offered to the parents of the other corners' parents
SDFK_TRI_HD inline int32_t hook_target(int32_t pa, int32_t pb, int32_t pc)
{
    const int32_t m = pa < pb ? pa : pb;
    return m < pc ? m : pc;
}
SDFK_TRI_HD inline bool hook_changes(int32_t old_parent, int32_t offered) { return old_parent > offered; }
// A launch after which nothing changed leaves the forest flat (a shortcut launch) or finished (a hook round on a flat forest).
// A component's root is then its lowest vertex; components are numbered by ascending root, which is the exclusive count of the
// roots below it.
SDFK_TRI_HD inline bool is_root(int32_t v, int32_t parent_v, bool referenced) { return referenced && parent_v == v; }
// the host's bound on the hook rounds: every round that changes something removes a tree
SDFK_TRI_HD inline int64_t max_rounds(int64_t nv) { return nv + 1; }

// ---- select -------------------------------------------------------------------------------------------------------------------
// label -1 (an index-degenerate triangle, an unreferenced vertex) is never kept
SDFK_TRI_HD inline bool keeps(int32_t label, const uint8_t* keep_component) { return label >= 0 && keep_component[label] != 0; }

// ---- derived on the host from a row (or the census: its column 0 is then the triangle count the caller supplies) --------------
inline int64_t euler_characteristic(int64_t vertices, int64_t edges, int64_t triangles) { return vertices - edges + triangles; }
inline bool is_watertight(const int64_t row[8]) { return row[kOdd] == 0; }
inline bool is_oriented(const int64_t row[8]) { return row[kInconsistent] == 0 && row[kNonManifold] == 0; }

// RemoveSmallComponents' rule, and LargestComponent's order
inline bool keep_by_size(const int64_t row[8], int64_t min_triangles, double min_area_fraction, int64_t total_weight)
{
    return row[kTriangles] >= min_triangles && (double)row[kAreaWeight] >= (double)min_area_fraction * (double)total_weight;
}
inline bool larger_than(const int64_t a[8], const int64_t b[8])   // (strictly: a tie leaves the lower number)
{
    if (a[kAreaWeight] != b[kAreaWeight]) return a[kAreaWeight] > b[kAreaWeight];
    return a[kTriangles] > b[kTriangles];
}

}  // namespace sdfk_trimesh_topo
