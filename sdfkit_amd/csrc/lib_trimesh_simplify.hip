// lib_trimesh_simplify.hip -- sdfk_trimesh_simplify*: vertex clustering.  The vertices of a handle's mesh grouped by the cell of a
// lattice exactly as sdfk_trimesh_weld groups them, every group replaced by one MADE vertex (its lowest index, the centroid, or
// the minimiser of the quadric of its triangles), the triangles rewritten, those that fall on top of each other cleaned up, and
// the mesh renumbered.  Contract: include/sdfkit_hip.h, "Triangle meshes: simplification".  Decisions and arithmetic:
// trimesh_simplify.h (shared with a host test).  The handle: trimesh_handle.h; it is not changed, but for the corner lists of the
// adjacency the quadric placement walks, which the handle keeps by contract.  Every decision is made on integers; no float
// atomics; every sum runs inside one lane in the stated order.
//
//   trimesh_groups   (lib_trimesh_weld.hip) bounds, keys, the sort, heads, the scan, rep -- and the vertex of every sorted position.
//   k_ts_is_rep      1 at every representative; one scan numbers the groups by ascending representative (the keys of the triangles).
//   k_ts_starts      the first sorted position of every run of a scanned head array (the members of a group; a run of triangles).
//   k_ts_tri_keys    one record (lo, index = t) per triangle: the least group number of its corners; index-degenerate ones are
//                    counted (a ballot per wave, one integer atomic) and carry the triple (0, 0, 0).
//   radix sort       device_sort.h, twice as welding's exact mode sorts 96 bits: by lo, then k_ts_tri_rekey gives every sorted
//                    record (hi above mid) and keeps lo in the record's spare word, and the second stable sort keeps the order of
//                    the first among equals.  Passes: the bytes a group number can set.
//   k_ts_tri_heads   head flag of every sorted record (another vertex set than its predecessor's); one scan numbers the runs.
//   k_ts_tri_runs    the keep flag of every triangle from its place in its run and the run's length; a kept one stores the byte 1
//                    at its three representatives.  (SDFK_SIMPLIFY_KEEP_DUPLICATES: k_ts_tri_plain, no sort.)
//   k_ts_vert_flags  keep flag of every vertex; two scans.
//   k_ts_place       THE HOT PATH: one lane per group, group -> members -> corners (trimesh_simplify.h place_group): the chunked
//                    binary64 centroid, the quadric of the incident triangles, the 3x3 eigen-solve, the cell test; the fallbacks
//                    are counted by a ballot per wave and one integer atomic.  A group that is not kept computes nothing.
//   k_ts_vertices / k_ts_triangles   vertex_map, vertex_index and the renumbered triangles.
// Host side: the scratch and the host form's device copies are held in a Staged (device_stage.h); the handle check
// (trimesh_check) and the launch size (grid1) are trimesh_handle.h's.
#include "lib_internal.h"
#include "device_scan.h"
#include "device_sort.h"
#include "device_wave.h"
#include "trimesh_handle.h"
#include "trimesh_simplify.h"

namespace {

using namespace sdfk_trimesh_simp;

constexpr int kBlock = 256;

struct Ctl {
    unsigned long long degenerate;   // index-degenerate triangles
    unsigned long long fallbacks;    // kept groups whose quadric placement fell back to the centroid
};

struct SimplifyOut {
    int32_t* vertex_map;
    int32_t* vertex_index;
    int32_t* triangle_index;
    int32_t* triangles;
    float* vertices;
    float* colors;
};

// counter += the wave's lanes whose flag is set
__device__ __forceinline__ void count_flagged(bool flag, unsigned long long* counter)
{
    const unsigned n = wave_count(flag);
    if (n && (threadIdx.x & 63) == 0) atomicAdd(counter, (unsigned long long)n);
}

// ---- groups -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ts_is_rep(const int32_t* __restrict__ rep, int64_t nv, uint32_t* __restrict__ flag)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v < nv) flag[v] = rep[v] == v ? 1u : 0u;
}

// head: scanned (head[n] = the number of runs); start: n + 1 entries, start[run] = its first position, start[runs] = n
__global__ __launch_bounds__(kBlock) void k_ts_starts(const uint32_t* __restrict__ head, int64_t n, uint32_t* __restrict__ start)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = head[j];
    if (head[j + 1] != r && r < n) start[r] = (uint32_t)j;   // (r < runs <= n)
    if (j == 0 && head[n] <= n) start[head[n]] = (uint32_t)n;
}

// ---- triangles --------------------------------------------------------------------------------------------------------------
// gnum: the scanned representative flags (gnum[rep[v]]: the number of v's group)
__device__ __forceinline__ Triple triple_of(const int32_t* __restrict__ idx, int64_t t, const int32_t* __restrict__ rep, const uint32_t* __restrict__ gnum)
{
    return sorted_triple(gnum[rep[idx[3 * t]]], gnum[rep[idx[3 * t + 1]]], gnum[rep[idx[3 * t + 2]]]);
}

__global__ __launch_bounds__(kBlock) void k_ts_tri_keys(const int32_t* __restrict__ idx, int64_t nt, const int32_t* __restrict__ rep,
                                                        const uint32_t* __restrict__ gnum, Rec* __restrict__ rec, Ctl* ctl)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool degenerate = false;
    if (t < nt) {
        const Triple s = triple_of(idx, t, rep, gnum);
        degenerate = !has_vertex_set(s);
        if (rec) rec[t] = Rec{triple_key_first(s), (uint32_t)t, 0u};
    }
    count_flagged(degenerate, &ctl->degenerate);
}

__global__ __launch_bounds__(kBlock) void k_ts_tri_rekey(const int32_t* __restrict__ idx, int64_t nt, const int32_t* __restrict__ rep,
                                                         const uint32_t* __restrict__ gnum, Rec* __restrict__ s)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nt) return;
    const uint32_t t = s[j].index;
    if (t >= nt) return;   // (never: the indices are 0 .. nt - 1)
    const Triple k = triple_of(idx, t, rep, gnum);
    s[j] = Rec{triple_key_second(k), t, k.lo};
}

__global__ __launch_bounds__(kBlock) void k_ts_tri_heads(const Rec* __restrict__ s, int64_t nt, uint32_t* __restrict__ head)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nt) return;
    const bool same = j > 0 && same_set(s[j].key, s[j].pad, s[j - 1].key, s[j - 1].pad);
    head[j] = sdfk_trimesh_wld::is_head(j, same) ? 1u : 0u;
}

__device__ __forceinline__ void mark_used(const int32_t* __restrict__ idx, int64_t t, const int32_t* __restrict__ rep, uint8_t* __restrict__ used)
{
    for (int k = 0; k < 3; k++) used[rep[idx[3 * t + k]]] = 1;   // (every writer stores the same byte)
}

// head: scanned; start: the runs' first positions (k_ts_starts)
__global__ __launch_bounds__(kBlock) void k_ts_tri_runs(const Rec* __restrict__ s, int64_t nt, const uint32_t* __restrict__ head,
                                                        const uint32_t* __restrict__ start, int32_t flags, const int32_t* __restrict__ idx,
                                                        const int32_t* __restrict__ rep, uint32_t* __restrict__ tflag, uint8_t* __restrict__ used)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nt) return;
    const uint32_t t = s[j].index, r = head[j];
    if (t >= nt) return;   // (never)
    const bool first = head[j + 1] != r;
    const uint32_t run = first && r < nt ? start[r + 1] - (uint32_t)j : 0u;
    const bool set = s[j].key != 0ull;   // (hi != 0: has_vertex_set)
    const bool keep = keeps_in_run(set, first, run, flags);
    tflag[t] = keep ? 1u : 0u;
    if (keep) mark_used(idx, t, rep, used);
}

// SDFK_SIMPLIFY_KEEP_DUPLICATES
__global__ __launch_bounds__(kBlock) void k_ts_tri_plain(const int32_t* __restrict__ idx, int64_t nt, const int32_t* __restrict__ rep,
                                                         uint32_t* __restrict__ tflag, uint8_t* __restrict__ used)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const bool keep = !index_degenerate(rep[idx[3 * t]], rep[idx[3 * t + 1]], rep[idx[3 * t + 2]]);
    tflag[t] = keep ? 1u : 0u;
    if (keep) mark_used(idx, t, rep, used);
}

// ---- vertices ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ts_vert_flags(const int32_t* __restrict__ rep, const uint8_t* __restrict__ used, int64_t nv,
                                                          uint32_t* __restrict__ vflag)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v < nv) vflag[v] = keeps_group((int32_t)v, rep[v], used[v] != 0) ? 1u : 0u;
}

struct Members {
    const uint32_t* order;
    __device__ __forceinline__ uint32_t operator()(int64_t i) const { return order[i]; }
};

// One lane per group (in sorted order); gstart: the groups' first sorted positions (k_ts_starts); vnew: the scanned vertex flags.
// The loops run over the lane's own group: its members, and their corners.
__global__ __launch_bounds__(kBlock) void k_ts_place(int64_t groups, int64_t nv, const uint32_t* __restrict__ order, const uint32_t* __restrict__ gstart,
                                                     const uint32_t* __restrict__ vnew, int32_t placement, float cell,
                                                     const float* __restrict__ pos, const float* __restrict__ col, const int32_t* __restrict__ idx,
                                                     const uint32_t* __restrict__ inc_start, const uint32_t* __restrict__ inc, SimplifyOut O, Ctl* ctl)
{
    const int64_t grp = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool fallback = false;
    if (grp < groups) {
        const uint32_t begin = gstart[grp], end = gstart[grp + 1];
        if (begin < end && end <= nv) {   // (always)
            const int64_t r = order[begin];   // the representative: the members ascend
            const int64_t o = vnew[r];
            if (vnew[r + 1] != o && o < nv) {
                float p[3], c[3];
                fallback = place_group(placement, pos, col, idx, inc_start, inc, cell, Members{order + begin}, (int64_t)(end - begin), p, c);
                if (O.vertices) __builtin_memcpy(O.vertices + 3 * o, p, sizeof p);   // (as bits)
                if (O.colors) __builtin_memcpy(O.colors + 3 * o, c, sizeof c);
            }
        }
    }
    count_flagged(fallback, &ctl->fallbacks);
}

__global__ __launch_bounds__(kBlock) void k_ts_vertices(const uint32_t* __restrict__ vnew, const int32_t* __restrict__ rep, int64_t nv, SimplifyOut O)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const int64_t r = rep[v];
    const int64_t o = vnew[r];
    const bool kept = vnew[r + 1] != o;
    if (O.vertex_map) O.vertex_map[v] = sdfk_trimesh_wld::map_of(kept, (uint32_t)o);
    if (r == v && kept && o < nv && O.vertex_index) O.vertex_index[o] = (int32_t)v;
}

__global__ __launch_bounds__(kBlock) void k_ts_triangles(const uint32_t* __restrict__ tnew, int64_t nt, const uint32_t* __restrict__ vnew,
                                                         const int32_t* __restrict__ rep, const int32_t* __restrict__ idx, SimplifyOut O)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const int64_t o = tnew[t];
    if (tnew[t + 1] == o || o >= nt) return;
    if (O.triangle_index) O.triangle_index[o] = (int32_t)t;
    if (O.triangles)
        for (int k = 0; k < 3; k++) O.triangles[3 * o + k] = (int32_t)vnew[rep[idx[3 * t + k]]];   // (a kept triangle's representatives are kept)
}

// ---- host -------------------------------------------------------------------------------------------------------------------
int check(const sdfk_trimesh* t, float cell, int32_t placement, int32_t flags, const char* who)
{
    if (int r = trimesh_check(t, who, 6)) return r;   // (what the adjacency asks)
    if (!cell_is_valid(cell)) return fail(SDFK_ERR_INVALID, "%s: cellSize must be finite and greater than 0", who);
    if (!placement_is_valid(placement)) return fail(SDFK_ERR_INVALID, "%s: unknown placement", who);
    if (!flags_are_known(flags)) return fail(SDFK_ERR_INVALID, "%s: unknown flag bits", who);
    if (!flags_are_compatible(flags)) return fail(SDFK_ERR_INVALID, "%s: KEEP_DUPLICATES and CANCEL_PAIRS exclude each other", who);
    return SDFK_OK;
}

// O: device buffers (any may be null); synchronises: the counts and stats are read on the way
int simplify(sdfk_trimesh* t, float cell, int32_t placement, int32_t flags, SimplifyOut O, int64_t* nv_out, int64_t* nt_out, int64_t stats[6],
             const char* who)
{
    const int64_t nv = t->nv, nt = t->nt;
    Staged st;
    TrimeshGroups G{};
    trimesh_groups(t, cell, true, st, &G, who);
    uint32_t groups = 0;
    st.read(&groups, G.head ? G.head + nv : nullptr, sizeof groups);
    if (placement == kQuadric) st.run([&] { return trimesh_corners(t, who); });
    Ctl* ctl = st.scratch<Ctl>(1);
    uint32_t* gstart = st.scratch<uint32_t>((size_t)nv + 1);
    uint32_t* gnum = st.scratch<uint32_t>((size_t)nv + 1);
    uint8_t* used = st.scratch<uint8_t>((size_t)nv);
    uint32_t* vnew = st.scratch<uint32_t>((size_t)nv + 1);
    uint32_t* tnew = st.scratch<uint32_t>((size_t)nt + 1);
    const bool sorts = !(flags & kKeepDuplicates);
    Rec* ra = sorts ? st.scratch<Rec>((size_t)nt) : nullptr;
    Rec* rb = sorts ? st.scratch<Rec>((size_t)nt) : nullptr;
    Rec* sorted = nullptr;
    uint32_t* thead = sorts ? st.scratch<uint32_t>((size_t)nt + 1) : nullptr;
    uint32_t* tstart = sorts ? st.scratch<uint32_t>((size_t)nt + 1) : nullptr;
    Ctl host{0ull, 0ull};
    uint32_t counts[2] = {0, 0};   // kept vertices, kept triangles
    st.run([&] { return hipMemsetAsync(ctl, 0, sizeof(Ctl), g.stream); });
    st.run([&] { return hipMemsetAsync(used, 0, (size_t)nv, g.stream); });
    {
        ProfScope ps("k_ts_groups");
        st.run([&] {
            hipLaunchKernelGGL(k_ts_starts, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, G.head, nv, gstart);
            hipLaunchKernelGGL(k_ts_is_rep, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, G.rep, nv, gnum);
        });
        st.run([&] { return sdfk_scan::scan(gnum, nv, who); });
    }
    st.run([&] {
        ProfScope ps("k_ts_tri_keys");
        hipLaunchKernelGGL(k_ts_tri_keys, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->idx, nt, G.rep, gnum, ra, ctl);
    });
    if (sorts) {
        st.run([&] { return radix_sort(ra, rb, nt, triple_mask_first(groups), &sorted, who); });
        st.run([&] {
            ProfScope ps("k_ts_tri_rekey");
            hipLaunchKernelGGL(k_ts_tri_rekey, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->idx, nt, G.rep, gnum, sorted);
        });
        st.run([&] { return radix_sort(sorted, sorted == ra ? rb : ra, nt, triple_mask_second(groups), &sorted, who); });
        ProfScope ps("k_ts_tri_runs");
        st.run([&] { hipLaunchKernelGGL(k_ts_tri_heads, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, sorted, nt, thead); });
        st.run([&] { return sdfk_scan::scan(thead, nt, who); });
        st.run([&] {
            hipLaunchKernelGGL(k_ts_starts, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, thead, nt, tstart);
            hipLaunchKernelGGL(k_ts_tri_runs, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, sorted, nt, thead, tstart, flags, t->idx, G.rep, tnew, used);
        });
    } else {
        st.run([&] {
            ProfScope ps("k_ts_tri_plain");
            hipLaunchKernelGGL(k_ts_tri_plain, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->idx, nt, G.rep, tnew, used);
        });
    }
    {
        ProfScope ps("k_ts_flags");
        st.run([&] { hipLaunchKernelGGL(k_ts_vert_flags, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, G.rep, used, nv, vnew); });
        st.run([&] { return sdfk_scan::scan(vnew, nv, who); });
        st.run([&] { return sdfk_scan::scan(tnew, nt, who); });
    }
    st.run([&] {
        ProfScope ps("k_ts_place");
        hipLaunchKernelGGL(k_ts_place, dim3(grid1(groups)), dim3(kBlock), 0, g.stream, (int64_t)groups, nv, G.order, gstart, vnew, placement, cell,
                           t->vertices, t->colors, t->idx, t->inc_start, t->inc, O, ctl);
    });
    {
        ProfScope ps("k_ts_output");
        st.run([&] {
            hipLaunchKernelGGL(k_ts_vertices, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, vnew, G.rep, nv, O);
            hipLaunchKernelGGL(k_ts_triangles, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, tnew, nt, vnew, G.rep, t->idx, O);
        });
        st.run([&] { return hipMemcpyAsync(&counts[0], vnew + nv, sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream); });
        st.run([&] { return hipMemcpyAsync(&counts[1], tnew + nt, sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream); });
        st.run([&] { return hipMemcpyAsync(&host, ctl, sizeof host, hipMemcpyDeviceToHost, g.stream); });
    }
    if (int r = st.finish(who)) return r;   // (synchronises: the counts are read)
    if (nv_out) *nv_out = counts[0];
    if (nt_out) *nt_out = counts[1];
    if (stats) {
        stats[kStatMerged] = nv - (int64_t)groups;
        stats[kStatDegenerate] = (int64_t)host.degenerate;
        stats[kStatDuplicates] = nt - (int64_t)host.degenerate - (int64_t)counts[1];
        stats[kStatUnreferenced] = (int64_t)groups - (int64_t)counts[0];
        stats[kStatPasses] = G.passes + triangle_passes(groups, flags);
        stats[kStatFallbacks] = (int64_t)host.fallbacks;
    }
    return SDFK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_trimesh_simplify_device(sdfk_trimesh* t, float cellSize, int32_t placement, int32_t flags, void* vertex_map_dev,
                                            void* vertex_index_out_dev, void* triangle_index_out_dev, void* triangles_out_dev, void* vertices_out_dev,
                                            void* colors_out_dev, int64_t* nv_out, int64_t* nt_out, int64_t stats[6])
{
    static const char* who = "sdfk_trimesh_simplify";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check(t, cellSize, placement, flags, who)) return r;
    return simplify(t, cellSize, placement, flags,
                    SimplifyOut{(int32_t*)vertex_map_dev, (int32_t*)vertex_index_out_dev, (int32_t*)triangle_index_out_dev, (int32_t*)triangles_out_dev,
                                (float*)vertices_out_dev, (float*)colors_out_dev},
                    nv_out, nt_out, stats, who);
}

extern "C" int sdfk_trimesh_simplify(sdfk_trimesh* t, float cellSize, int32_t placement, int32_t flags, int32_t* vertex_map, int32_t* vertex_index_out,
                                     int32_t* triangle_index_out, int32_t* triangles_out, float* vertices_out, float* colors_out, int64_t* nv_out,
                                     int64_t* nt_out, int64_t stats[6])
{
    static const char* who = "sdfk_trimesh_simplify";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check(t, cellSize, placement, flags, who)) return r;
    const size_t nv = (size_t)t->nv, nt = (size_t)t->nt;
    Staged st;
    const SimplifyOut O{st.out(vertex_map, nv), vertex_index_out ? st.scratch<int32_t>(nv) : nullptr,
                        triangle_index_out ? st.scratch<int32_t>(nt) : nullptr, triangles_out ? st.scratch<int32_t>(3 * nt) : nullptr,
                        vertices_out ? st.scratch<float>(3 * nv) : nullptr, colors_out ? st.scratch<float>(3 * nv) : nullptr};
    int64_t kv = 0, kt = 0, stv[kStats] = {0, 0, 0, 0, 0, 0};
    st.run([&] { return simplify(t, cellSize, placement, flags, O, &kv, &kt, stv, who); });   // (synchronises: the counts size the copies back)
    st.run([&] { return copy_out(vertex_index_out, O.vertex_index, (size_t)kv); });   // (the kept ones only: the rest of the caller's arrays stays)
    st.run([&] { return copy_out(triangle_index_out, O.triangle_index, (size_t)kt); });
    st.run([&] { return copy_out(triangles_out, O.triangles, 3 * (size_t)kt); });
    st.run([&] { return copy_out(vertices_out, O.vertices, 3 * (size_t)kv); });
    st.run([&] { return copy_out(colors_out, O.colors, 3 * (size_t)kv); });
    if (int r = st.finish(who)) return r;
    if (nv_out) *nv_out = kv;
    if (nt_out) *nt_out = kt;
    if (stats)
        for (int k = 0; k < kStats; k++) stats[k] = stv[k];
    return SDFK_OK;
}
