// trimesh_handle.h -- the handle behind sdfk_trimesh_*: the copied arrays, the packed triangles and their search grid (built by
// lib_trimesh.hip), the sampling weights' scan (made by the first call that needs it) and the component labels (made by the first
// topology call, lib_trimesh_topology.hip) and the adjacency (made by the first adjacency, smoothing or vertex-normal call,
// lib_trimesh_smooth.hip).  Seen by those three translation units and by lib_trimesh_weld.hip, lib_trimesh_simplify.hip and
// lib_trimesh_ray.hip, which only read it (simplification asks for the corner lists of the adjacency; the ray caster walks the
// search grid), and by lib_trimesh_winding.hip, which keeps its hierarchy here.  With it, what the six share on the host: the staging of
// device_stage.h, the check of a handle, the size of a one-dimensional launch, and the grouping of the vertices by position.
// hipcc only.
#pragma once
#include "lib_internal.h"
#include "device_stage.h"
#include "points_grid.h"

#include <algorithm>

// packed triangle: a, b, c (f32) and the AABB
struct TriPack {
    float4 p0;   // ax ay az bx
    float4 p1;   // by bz cx cy
    float4 p2;   // cz lox loy loz
    float4 p3;   // hix hiy hiz -
};

// the reader of the packed triangles: what the walks shared with the host tests (trimesh_ray.h, trimesh_winding.h) take as their
// triangle source, and what a kernel unpacks a TriPack with
struct PackTris {
    const TriPack* tri;
    __device__ __forceinline__ void box(uint32_t t, float lo[3], float hi[3]) const
    {
        const float4 p2 = tri[t].p2, p3 = tri[t].p3;
        lo[0] = p2.y; lo[1] = p2.z; lo[2] = p2.w;
        hi[0] = p3.x; hi[1] = p3.y; hi[2] = p3.z;
    }
    __device__ __forceinline__ void corners(uint32_t t, float a[3], float b[3], float c[3]) const
    {
        const float4 p0 = tri[t].p0, p1 = tri[t].p1;
        a[0] = p0.x; a[1] = p0.y; a[2] = p0.z;
        b[0] = p0.w; b[1] = p1.x; b[2] = p1.y;
        c[0] = p1.z; c[1] = p1.w; c[2] = tri[t].p2.x;
    }
};

struct sdfk_trimesh {
    DeviceState* owner = &cur_state();
    int64_t nv = 0, nt = 0;
    float* vertices = nullptr;      // nv x 3
    float* colors = nullptr;        // nv x 3, or null
    int32_t* idx = nullptr;         // nt x 3
    TriPack* tri = nullptr;         // nt
    uint32_t* list = nullptr;       // entries: triangle indices in cell order
    uint32_t* starts = nullptr;     // cells + 1, x-fastest
    uint32_t* ystarts = nullptr;    // cells + 1, y-fastest
    int64_t cells = 0, entries = 0;
    sdfk_points_grid::Grid G{};
    int64_t last_candidates = 0, last_queries = 0, last_crossings = 0;
    unsigned long long* sample_W = nullptr;   // nt + 1: the exclusive scan of the sampling weights (made by the first call that needs them)
    int64_t sample_nonzero = 0, sample_total = 0;
    bool sample_no_area = false;              // no triangle has an area: W is all zeros, and sampling is refused
    int32_t* comp_vertex = nullptr;           // nv: the component of every vertex, -1: none (made by the first topology call)
    int32_t* comp_triangle = nullptr;         // nt
    int64_t comp_count = 0, comp_rounds = 0, comp_shortcuts = 0;
    uint32_t* nbr_start = nullptr;            // nv + 1: the neighbours of v are nbr[nbr_start[v] .. nbr_start[v + 1]), ascending, each once
    uint32_t* nbr = nullptr;                  // nbr_entries
    uint8_t* boundary = nullptr;              // nv: 1 for the endpoints of an edge with one triangle side
    uint32_t* inc_start = nullptr;            // nv + 1: the corners 3 t + k of v are inc[inc_start[v] .. inc_start[v + 1]), ascending
    uint32_t* inc = nullptr;                  // 3 nt (inc_entries of them used)
    int64_t nbr_entries = 0, inc_entries = 0;
    void* wn_nodes = nullptr;                 // the nodes of the winding-number hierarchy (sdfk_trimesh_wn::Node; made by the first winding call)
    uint32_t* wn_order = nullptr;             // nt: the triangles sorted by (cell code, index)
    int wn_levels = -1;                       // L; -1: no hierarchy yet
    int64_t wn_occupied = 0, wn_max_leaf = 0, wn_builds = 0;
    int64_t last_wn_clusters = 0, last_wn_triangles = 0, last_wn_queries = 0;
};

// The count of a profiled call (the candidates of a search, the triangle tests of a ray cast) and its queries onto the handle, for
// sdfk_trimesh_stats; nothing when the call was not profiled or has failed.  Ends pc: synchronises.
inline void trimesh_keep_count(Staged& st, ProfCount<1>& pc, const sdfk_trimesh* t, int64_t queries)
{
    unsigned long long c[1];
    if (!pc.end(st, c)) return;
    const_cast<sdfk_trimesh*>(t)->last_candidates = (int64_t)c[0];
    const_cast<sdfk_trimesh*>(t)->last_queries = queries;
}

// The sampling weights and their scan, once per handle (lib_trimesh.hip): synchronises to read the total.  A mesh in which no
// triangle has an area gets W = 0 everywhere and sample_no_area; refusing it is the sampler's business.
int trimesh_weights(sdfk_trimesh* t, const char* who);

// What every entry point of the family asks of its handle first: the library is initialised, t is not null, and -- for a unit
// that sorts `records` 32-bit-indexed records per triangle (0: none) -- records * nt < 2^32.  (lib_trimesh.hip)
int trimesh_check(const sdfk_trimesh* t, const char* who, int records);

// sdfk_trimesh_to_volume's work (lib_trimesh.hip; the arguments are checked).  sign_dev null: the parity of the crossings along z.
// Otherwise one byte per voxel in the order of the volume pass ((i * ny + j) * nz + k, unpadded), non-zero: inside -- the sign of
// lib_trimesh_winding.hip -- and no crossing records are made.
int trimesh_to_volume(const sdfk_trimesh* t, sdfk_volume* v, float band, const uint8_t* sign_dev);

// The vertices of a handle grouped by position as sdfk_trimesh_weld groups them (lib_trimesh_weld.hip; tolerance 0: equal as
// values, > 0: the cell of the lattice), for the units that start from the groups (welding itself, lib_trimesh_simplify.hip).  The
// steps are queued on st, which owns every array below and reports a refusal (an axis of 2^21 cells or more) or a failure at its
// finish(); nothing is kept on the handle.
struct TrimeshGroups {
    uint32_t* order;        // nv (want_order; else null): the vertex at every sorted position -- the members of a group are adjacent, ascending
    uint32_t* head;         // nv + 1: the scanned head flags of the sorted positions; head[nv] = the number of groups
    int32_t* group_first;   // nv: the lowest index of every group, the groups in sorted order
    int32_t* rep;           // nv: the lowest index of every vertex's group
    int passes;             // radix passes run
};
void trimesh_groups(const sdfk_trimesh* t, float tolerance, bool want_order, Staged& st, TrimeshGroups* G, const char* who);

// The corner lists inc_start / inc of the handle, made by the first call that needs them (lib_trimesh_smooth.hip); the caller has
// checked the handle for 6 records per triangle.
int trimesh_corners(sdfk_trimesh* t, const char* who);

// blocks of 256 lanes for n items, one lane each; at least one, at most 2^30 (reached by nothing indexed per vertex or triangle)
inline unsigned grid1(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, int64_t(1) << 30)); }
