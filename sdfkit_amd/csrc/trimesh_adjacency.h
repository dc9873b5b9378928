// trimesh_adjacency.h -- the arithmetic and the decisions of sdfk_trimesh_adjacency / _smooth / _vertex_normals
// (lib_trimesh_smooth.hip: per-vertex gathers over the incidence of a triangle mesh): the records of the two sorts and the passes
// they need, what a sorted position starts and ends, one smoothing step of one vertex, the normal of one vertex.  Plain C++
// outside hipcc, so that tests/cpp/mesh_smooth_host.cpp runs exactly the code the kernels run.  Compiled with -ffp-contract=off
// everywhere: no expression below may be fused.  Every sum runs over a vertex's own neighbours or corners in ascending order.
#pragma once
#include <cstdint>

#include "trimesh_sample.h"     // area2: the triangle's (b - a) x (c - a)
#include "trimesh_topology.h"   // index_degenerate, index_bytes

namespace sdfk_trimesh_adj {

using sdfk_trimesh_sdf::sq3;
using sdfk_trimesh_smp::area2;
using sdfk_trimesh_topo::index_bytes;
using sdfk_trimesh_topo::index_degenerate;

// ---- the records ----------------------------------------------------------------------------------------------------------------
// Neighbours: directed record j (0 .. 5) of the triangle (a, b, c): (a,b), (b,a), (b,c), (c,b), (c,a), (a,c); key = from << 32 | to.
// Corners: record k (0, 1, 2) of triangle t: key = the vertex, index = 3 t + k.
// An index-degenerate triangle writes the same number of records with the vertex nv, which no triangle names, in the place of
// `from`: they sort behind everything and belong to no vertex.
SDFK_TRI_HD inline void directed_record(const int32_t tri[3], int j, int32_t* from, int32_t* to)
{
    const int e = j >> 1, u = e, v = e == 2 ? 0 : e + 1;
    *from = tri[(j & 1) ? v : u];
    *to = tri[(j & 1) ? u : v];
}
SDFK_TRI_HD inline uint64_t nbr_key(int64_t from, int64_t to) { return (uint64_t)from << 32 | (uint64_t)to; }
SDFK_TRI_HD inline uint64_t nbr_skip_key(int64_t nv) { return (uint64_t)nv << 32; }
SDFK_TRI_HD inline uint64_t corner_skip_key(int64_t nv) { return (uint64_t)nv; }
// the vertex a sorted record belongs to (shift: 32 for the neighbours, 0 for the corners); nv: none
SDFK_TRI_HD inline int64_t record_vertex(uint64_t key, int shift) { return (int64_t)(key >> shift); }

// The passes of the two sorts: the bytes `to` can set (a vertex below nv) and the bytes `from` can set (a vertex, or nv).
SDFK_TRI_HD inline unsigned nbr_digit_mask(int64_t nv) { return ((1u << index_bytes(nv)) - 1u) | ((1u << index_bytes(nv + 1)) - 1u) << 4; }
SDFK_TRI_HD inline unsigned corner_digit_mask(int64_t nv) { return (1u << index_bytes(nv + 1)) - 1u; }

// the limit of both: 6 nt records are counted in 32 bits
SDFK_TRI_HD inline bool too_many_triangles(int64_t nt) { return 6 * nt >= (int64_t(1) << 32); }

// ---- what a sorted position is ----------------------------------------------------------------------------------------------------
// `prev` / `next`: the keys of the positions before and after (has_prev / has_next: whether there are such positions).
// An entry of the output list begins here: a record of a vertex whose key differs from the one before.  (Corner records all
// differ in their index, not their key: every one of them is an entry, and the caller does not ask.)
SDFK_TRI_HD inline bool entry_head(uint64_t key, bool has_prev, uint64_t prev, int64_t nv, int shift)
{
    return record_vertex(key, shift) < nv && (!has_prev || prev != key);
}
// the first / last record of its vertex
SDFK_TRI_HD inline bool vertex_first(uint64_t key, bool has_prev, uint64_t prev, int64_t nv, int shift)
{
    return record_vertex(key, shift) < nv && (!has_prev || record_vertex(prev, shift) != record_vertex(key, shift));
}
SDFK_TRI_HD inline bool vertex_last(uint64_t key, bool has_next, uint64_t next, int64_t nv, int shift)
{
    return record_vertex(key, shift) < nv && (!has_next || record_vertex(next, shift) != record_vertex(key, shift));
}
// A run of one record: the undirected edge {from, to} has one triangle side, a boundary edge.
SDFK_TRI_HD inline bool run_of_one(uint64_t key, bool has_prev, uint64_t prev, bool has_next, uint64_t next)
{
    return (!has_prev || prev != key) && (!has_next || next != key);
}

// ---- one smoothing step of vertex v -------------------------------------------------------------------------------------------------
// pos: the positions of the step before; nbr[begin .. end): v's neighbours, ascending.
SDFK_TRI_HD inline void smooth_vertex(const float* pos, const uint32_t* nbr, uint32_t begin, uint32_t end, bool pinned, float s, int64_t v, float out[3])
{
    if (begin == end || pinned) {
        __builtin_memcpy(out, pos + 3 * v, 3 * sizeof(float));   // (as bits)
        return;
    }
    const float* q = pos + 3 * (int64_t)nbr[begin];
    double acc[3] = {(double)q[0], (double)q[1], (double)q[2]};
    for (uint32_t i = begin + 1; i < end; i++) {
        q = pos + 3 * (int64_t)nbr[i];
        acc[0] += (double)q[0]; acc[1] += (double)q[1]; acc[2] += (double)q[2];
    }
    const double degree = (double)(end - begin);
    for (int k = 0; k < 3; k++) {
        const double p = (double)pos[3 * v + k];
        const double mean = acc[k] / degree;
        out[k] = (float)(p + (double)s * (mean - p));
    }
}

// the factor of step `step` (0, 1, ...) of a call, and the number of its steps
SDFK_TRI_HD inline int64_t smooth_steps(int32_t iterations, float mu) { return (int64_t)iterations * (mu != 0.0f ? 2 : 1); }
SDFK_TRI_HD inline float smooth_factor(int64_t step, float lambda, float mu) { return mu != 0.0f && (step & 1) ? mu : lambda; }

// ---- the normal of vertex v ---------------------------------------------------------------------------------------------------------
// inc[begin .. end): v's corners 3 t + k, ascending; the triangles' positions are gathered through idx.
SDFK_TRI_HD inline void vertex_normal(const float* pos, const int32_t* idx, const uint32_t* inc, uint32_t begin, uint32_t end, bool flip, float out[3])
{
    double sum[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = begin; i < end; i++) {
        const int32_t* tri = idx + 3 * (int64_t)(inc[i] / 3u);
        double n[3];
        area2(pos + 3 * (int64_t)tri[0], pos + 3 * (int64_t)tri[1], pos + 3 * (int64_t)tri[2], n);
        sum[0] += n[0]; sum[1] += n[1]; sum[2] += n[2];
    }
    const double len = __builtin_sqrt(sq3(sum));
    const bool usable = begin != end && len > 0.0 && len < __builtin_inf();
    for (int k = 0; k < 3; k++) {
        const double c = sum[k] / len;
        out[k] = usable ? (float)(flip ? -c : c) : 0.0f;
    }
}

}  // namespace sdfk_trimesh_adj
