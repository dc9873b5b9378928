// lib_points_cluster.hip -- the KdTree's density clustering: sdfk_points_cluster* (DBSCAN with a border rule that does not depend
// on any order; min_points = 1: Euclidean cluster extraction) and sdfk_points_select* (the points of the kept clusters).  Contract:
// include/sdfkit_hip.h, "Point clouds: clusters"; the decisions (within, count, core, hook, root, border choice, keep rule,
// argument checks): points_cluster.h, checked on the host; the walk and its launch: points_walk.h, shared with every query of the
// KdTree; the label rounds: device_forest.h; the scan of the roots and of the compaction: device_scan.h.  Everything accumulated
// is an integer; no float atomics; the result does not depend on the order the atomics land in.
//
// Cluster, one lane per static point:
//   k_cl_count     on the shell walk: the candidates within the radius, saturating; the core byte; parent[i] = i; the core total
//                  (summed over the wave, one atomic per wave).
//   k_cl_hook      a core point i on the same walk: for every core candidate j != i within the radius the hook of the edge on the
//                  two parents (relaxed atomic loads; atomicMin of the lower into the parent of the higher).  The lane keeps its
//                  own parent in a register and loads it again after a hook.  Every round repeats the walk: no edge is stored,
//                  the memory of a call is O(n).
//   k_forest_shortcut and the round driver: device_forest.h.
//   k_cl_roots     flags core_i && parent[i] == i; a scan numbers them (ascending root); the host reads C.
//   k_cl_labels    a core point gets number[parent[i]], any other -1 for now.
//   k_cl_border    a point that is not core on the walk: the least key among the core candidates within the radius; the walk
//                  stops by the k-nearest rule on that key.  Runs after the core labels are final: it reads those only and
//                  writes the others only.
//   k_cl_sizes     one integer add per member, border and noise totals; a wave whose lanes all name one cluster adds once.
// Select:
//   k_cs_flags     the keep rule per point; a scan; k_cs_scatter writes the kept indices and points.
// Host side: all per-call scratch and the host forms' device copies are held in a Staged (device_stage.h).
#include "lib_internal.h"
#include "device_forest.h"
#include "device_scan.h"
#include "points_cluster.h"
#include "points_knn.h"
#include "points_set.h"
#include "points_walk.h"

#include <climits>

namespace {

using namespace sdfk_walk;
using namespace sdfk_cluster;

typedef unsigned long long u64;

enum { kTotCore = 0, kTotBorder, kTotNoise, kTotals };

// ---- count ------------------------------------------------------------------------------------------------------------------
struct ClCountVisitor {
    uint64_t bound_key;
    float d2_bound;
    int32_t n;
    __device__ __forceinline__ void take(float d2, const float4& s)
    {
        if (reaches(pack_key(d2, __float_as_int(s.w)), bound_key)) n = count_add(n);
    }
    __device__ __forceinline__ bool done(float lb2) const { return walk_done(lb2, kKeyInf, d2_bound); }
};

__global__ __launch_bounds__(kBlock) void k_cl_count(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                     const float* __restrict__ xyz, int64_t n, float d2_bound, int32_t min_points,
                                                     int32_t* __restrict__ counts, uint8_t* __restrict__ core, int32_t* __restrict__ parent,
                                                     u64* totals, unsigned long long* candidates)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const Query q = load_query(xyz, t, n);
    ClCountVisitor v{pack_key(d2_bound, -1), d2_bound, 0};
    unsigned long long ncand = 0;
    if (q.finite) ncand = shell_walk(sorted, starts, G, q.x, q.y, q.z, v);
    const bool c = t < n && is_core(v.n, min_points);
    if (t < n) {
        if (counts) counts[t] = v.n;
        core[t] = c ? 1 : 0;
        parent[t] = (int32_t)t;
    }
    const u64 cores = wave_sum(c ? 1ull : 0ull);
    if ((threadIdx.x & 63) == 0 && cores) atomicAdd(&totals[kTotCore], cores);
    wave_add(candidates, ncand);
}

// ---- hook -------------------------------------------------------------------------------------------------------------------
struct ClHookVisitor {
    uint64_t bound_key;
    float d2_bound;
    int32_t i, pi;   // the lane's point and its parent as last loaded
    const uint8_t* core;
    int32_t* parent;
    unsigned changed;
    __device__ __forceinline__ void take(float d2, const float4& s)
    {
        const int32_t j = __float_as_int(s.w);
        if (j == i || !reaches(pack_key(d2, j), bound_key) || !core[j]) return;
        const int32_t pj = __atomic_load_n(&parent[j], __ATOMIC_RELAXED);
        int32_t at, offered;
        if (!hook_edge(pi, pj, &at, &offered)) return;
        if (hook_changes(atomicMin(&parent[at], offered), offered)) changed++;
        pi = __atomic_load_n(&parent[i], __ATOMIC_RELAXED);
    }
    __device__ __forceinline__ bool done(float lb2) const { return walk_done(lb2, kKeyInf, d2_bound); }
};

__global__ __launch_bounds__(kBlock) void k_cl_hook(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                    const float* __restrict__ xyz, int64_t n, float d2_bound, const uint8_t* __restrict__ core,
                                                    int32_t* parent, ForestCtl* ctl, int q, unsigned long long* candidates)
{
    forest_hook_begin(ctl, q);
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const Query p = load_query(xyz, t, n);
    unsigned long long ncand = 0;
    unsigned changed = 0;
    if (p.finite && core[t]) {   // (finite: t < n)
        ClHookVisitor v{pack_key(d2_bound, -1), d2_bound, (int32_t)t, __atomic_load_n(&parent[t], __ATOMIC_RELAXED), core, parent, 0u};
        ncand = shell_walk(sorted, starts, G, p.x, p.y, p.z, v);
        changed = v.changed;
    }
    forest_hook_end(ctl, q, changed);
    wave_add(candidates, ncand);
}

// ---- labels -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_cl_roots(const int32_t* __restrict__ parent, const uint8_t* __restrict__ core, int64_t n,
                                                     uint32_t* __restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    flag[i] = is_root((int32_t)i, parent[i], core[i] != 0) ? 1u : 0u;
}

// number: the scanned root flags (number[r] of a root r = its cluster)
__global__ __launch_bounds__(kBlock) void k_cl_labels(const int32_t* __restrict__ parent, const uint8_t* __restrict__ core, int64_t n,
                                                      const uint32_t* __restrict__ number, int32_t* __restrict__ label)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    label[i] = core[i] ? (int32_t)number[parent[i]] : -1;
}

// ---- border -----------------------------------------------------------------------------------------------------------------
struct ClBorderVisitor {
    uint64_t bound_key, best;
    float d2_bound;
    const uint8_t* core;
    __device__ __forceinline__ void take(float d2, const float4& s)
    {
        const int32_t j = __float_as_int(s.w);
        const uint64_t key = pack_key(d2, j);
        if (reaches(key, bound_key) && key < best) best = border_take(best, key, bound_key, core[j] != 0);   // (core[j] is read only where it decides)
    }
    __device__ __forceinline__ bool done(float lb2) const { return walk_done(lb2, best, d2_bound); }
};

// label: final at the core points (read there only), written at the others only
__global__ __launch_bounds__(kBlock) void k_cl_border(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                      const float* __restrict__ xyz, int64_t n, float d2_bound, const uint8_t* __restrict__ core,
                                                      int32_t* label, unsigned long long* candidates)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const Query p = load_query(xyz, t, n);
    unsigned long long ncand = 0;
    if (p.finite && !core[t]) {   // (a point with a coordinate that is not finite has no neighbour: -1 already)
        ClBorderVisitor v{pack_key(d2_bound, -1), kKeyInf, d2_bound, core};
        ncand = shell_walk(sorted, starts, G, p.x, p.y, p.z, v);
        const int32_t from = border_source(v.best);
        if (from >= 0 && from < n) label[t] = label[from];
    }
    wave_add(candidates, ncand);
}

// ---- sizes ------------------------------------------------------------------------------------------------------------------
// Every lane of the wave comes here.  c: the lane's cluster, -1: none.  -> whether the lanes that have one all name the same
// (*c0), so that lane 0 may add the wave's sum to that entry.
__device__ __forceinline__ bool wave_uniform(int32_t c, int32_t* c0)
{
    const u64 valid = __ballot(c >= 0);
    *c0 = -1;
    if (!valid) return false;
    *c0 = __shfl(c, __ffsll((long long)valid) - 1);
    return __ballot(c >= 0 && c != *c0) == 0;
}

__global__ __launch_bounds__(kBlock) void k_cl_sizes(const int32_t* __restrict__ label, const uint8_t* __restrict__ core, int64_t n, int64_t C,
                                                     int32_t* sizes, u64* totals)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t c = i < n ? label[i] : -1;
    const bool noise = i < n && c < 0, border = i < n && c >= 0 && !core[i];
    if (c >= C) c = -1;   // (never: a label is below C)
    const u64 nb = wave_sum(border ? 1ull : 0ull), nn = wave_sum(noise ? 1ull : 0ull);
    if ((threadIdx.x & 63) == 0) {
        if (nb) atomicAdd(&totals[kTotBorder], nb);
        if (nn) atomicAdd(&totals[kTotNoise], nn);
    }
    if (!sizes) return;
    int32_t c0;
    const bool uniform = wave_uniform(c, &c0);
    if (c0 < 0) return;
    if (uniform) {
        const u64 members = wave_sum(c >= 0 ? 1ull : 0ull);
        if ((threadIdx.x & 63) == 0) atomicAdd(&sizes[c0], (int32_t)members);
    } else if (c >= 0)
        atomicAdd(&sizes[c], 1);
}

// ---- select -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_cs_flags(const int32_t* __restrict__ label, int64_t n, const uint8_t* __restrict__ keep,
                                                     int64_t n_clusters, uint32_t* __restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    flag[i] = keeps(label[i], n_clusters, keep) ? 1u : 0u;
}

// flag: scanned (flag[i + 1] != flag[i]: i is kept, as output flag[i])
__global__ __launch_bounds__(kBlock) void k_cs_scatter(const uint32_t* __restrict__ flag, int64_t n, const float* __restrict__ xyz,
                                                       int32_t* __restrict__ index_out, float* __restrict__ points_out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t o = flag[i];
    if (flag[i + 1] == o || o >= n) return;
    if (index_out) index_out[o] = (int32_t)i;
    if (points_out)
        for (int a = 0; a < 3; a++) points_out[3 * o + a] = xyz[3 * i + a];
}

// ---- host -------------------------------------------------------------------------------------------------------------------
int check_cluster(const sdfk_points* s, float radius, int32_t min_points)
{
    static const char* who = "sdfk_points_cluster";
    if (int r = require_init()) return r;
    switch (check_cluster_args(s != nullptr, radius, min_points)) {
    case kArgsOk: return SDFK_OK;
    case kArgsNullSet: return fail(SDFK_ERR_INVALID, "%s: null point set", who);
    case kArgsRadius: return fail(SDFK_ERR_INVALID, "%s: the radius is negative or NaN", who);
    default: return fail(SDFK_ERR_INVALID, "%s: min_points = %d is below 1", who, (int)min_points);
    }
}

int check_select(const sdfk_points* s, const void* labels, const void* keep, int64_t n_clusters)
{
    static const char* who = "sdfk_points_select";
    if (int r = require_init()) return r;
    switch (check_select_args(s != nullptr, labels != nullptr, keep != nullptr, n_clusters)) {
    case kArgsOk: return SDFK_OK;
    case kArgsNullSet: return fail(SDFK_ERR_INVALID, "%s: null point set", who);
    case kArgsNullLabels: return fail(SDFK_ERR_INVALID, "%s: null labels", who);
    case kArgsClusterCount: return fail(SDFK_ERR_INVALID, "%s: n_clusters = %lld is negative", who, (long long)n_clusters);
    default: return fail(SDFK_ERR_INVALID, "%s: null keep bytes for %lld clusters", who, (long long)n_clusters);
    }
}

// everything on the device; C is read on the way (the call is synchronous).  Any output may be null.
int cluster(const sdfk_points* s, float radius, int32_t min_points, int32_t* labels, int32_t* sizes, uint8_t* core, int32_t* counts,
            int64_t* n_clusters, int64_t stats[6])
{
    static const char* who = "sdfk_points_cluster";
    const int64_t n = s->n;
    const float d2b = radius_d2_bound(radius);
    Staged st;
    int32_t* parent = st.scratch<int32_t>((size_t)n);
    uint32_t* flag = st.scratch<uint32_t>((size_t)n + 1);
    if (!core) core = st.scratch<uint8_t>((size_t)n);
    if (!labels) labels = st.scratch<int32_t>((size_t)n);
    u64* totals = st.scratch<u64>(kTotals);
    ForestCtl* ctl = st.scratch<ForestCtl>(1);
    ForestCtl host{};
    int64_t candidates = 0;   // of every walk of the call, under profiling
    auto walk = [&](const char* name, auto&& launch) {
        const int r = walk_launch(s, n, name, who, launch);
        if (g.prof_on) candidates += s->last_candidates;
        return r;
    };
    const dim3 grid(grid_of(n, kBlock)), block(kBlock);
    st.run([&] { return hipMemsetAsync(totals, 0, kTotals * sizeof(u64), g.stream); });
    st.run([&] {
        return walk("k_cl_count", [&](unsigned long long* counter) {
            hipLaunchKernelGGL(k_cl_count, grid, block, 0, g.stream, s->sorted, s->starts, s->G, s->xyz, n, d2b, min_points, counts, core, parent, totals,
                               counter);
        });
    });
    forest_rounds(st, parent, n, ctl, &host, max_rounds(n), who, "k_cl_shortcut", [&](ForestCtl* c, int q) {
        return walk("k_cl_hook", [&](unsigned long long* counter) {
            hipLaunchKernelGGL(k_cl_hook, grid, block, 0, g.stream, s->sorted, s->starts, s->G, s->xyz, n, d2b, core, parent, c, q, counter);
        });
    });
    uint32_t C = 0;
    {
        ProfScope ps("k_cl_labels");
        st.run([&] { hipLaunchKernelGGL(k_cl_roots, grid, block, 0, g.stream, parent, core, n, flag); });
        st.run([&] { return sdfk_scan::scan(flag, n, who); });
        st.run([&] { hipLaunchKernelGGL(k_cl_labels, grid, block, 0, g.stream, parent, core, n, flag, labels); });
        st.read(&C, flag + n, sizeof C);
    }
    st.run([&] {
        return walk("k_cl_border", [&](unsigned long long* counter) {
            hipLaunchKernelGGL(k_cl_border, grid, block, 0, g.stream, s->sorted, s->starts, s->G, s->xyz, n, d2b, core, labels, counter);
        });
    });
    u64 tot[kTotals] = {0, 0, 0};
    {
        ProfScope ps("k_cl_sizes");
        if (sizes && C) st.run([&] { return hipMemsetAsync(sizes, 0, (size_t)C * sizeof(int32_t), g.stream); });   // (entries from C on stay)
        st.run([&] { hipLaunchKernelGGL(k_cl_sizes, grid, block, 0, g.stream, labels, core, n, (int64_t)C, sizes, totals); });
        st.read(tot, totals, sizeof tot);
    }
    if (int r = st.finish(who)) return r;   // (synchronises: the call returns when finished)
    if (g.prof_on) {
        const_cast<sdfk_points*>(s)->last_candidates = candidates;
        const_cast<sdfk_points*>(s)->last_queries = n;
    }
    if (n_clusters) *n_clusters = (int64_t)C;
    if (stats) {
        stats[0] = (int64_t)C;
        stats[1] = (int64_t)tot[kTotCore];
        stats[2] = (int64_t)tot[kTotBorder];
        stats[3] = (int64_t)tot[kTotNoise];
        stats[4] = (int64_t)host.rounds;
        stats[5] = (int64_t)host.shortcuts;
    }
    return SDFK_OK;
}

int select(const sdfk_points* s, const int32_t* labels, const uint8_t* keep, int64_t n_clusters, int32_t* index_out, float* points_out,
           int64_t* n_kept)
{
    static const char* who = "sdfk_points_select";
    const int64_t n = s->n;
    Staged st;
    uint32_t* flag = st.scratch<uint32_t>((size_t)n + 1);
    uint32_t kept = 0;
    {
        ProfScope ps("k_cs_select");
        const dim3 grid(grid_of(n, kBlock)), block(kBlock);
        st.run([&] { hipLaunchKernelGGL(k_cs_flags, grid, block, 0, g.stream, labels, n, keep, n_clusters, flag); });
        st.run([&] { return sdfk_scan::scan(flag, n, who); });
        if (index_out || points_out)
            st.run([&] { hipLaunchKernelGGL(k_cs_scatter, grid, block, 0, g.stream, flag, n, s->xyz, index_out, points_out); });
        st.read(&kept, flag + n, sizeof kept);
    }
    if (int r = st.finish(who)) return r;
    if (n_kept) *n_kept = (int64_t)kept;
    return SDFK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_points_cluster_device(const sdfk_points* s, float radius, int32_t min_points, void* labels_dev, void* sizes_dev, void* core_dev,
                                          void* counts_dev, int64_t* n_clusters, int64_t stats[6])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_cluster(s, radius, min_points)) return r;
    return cluster(s, radius, min_points, (int32_t*)labels_dev, (int32_t*)sizes_dev, (uint8_t*)core_dev, (int32_t*)counts_dev, n_clusters, stats);
}

extern "C" int sdfk_points_cluster(const sdfk_points* s, float radius, int32_t min_points, int32_t* labels, int32_t* sizes, uint8_t* core,
                                   int32_t* counts, int64_t* n_clusters, int64_t stats[6])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_cluster(s, radius, min_points)) return r;
    const size_t n = (size_t)s->n;
    Staged st;
    int32_t* labels_d = st.out(labels, n);
    uint8_t* core_d = st.out(core, n);
    int32_t* counts_d = st.out(counts, n);
    int32_t* sizes_d = sizes ? st.scratch<int32_t>(n) : nullptr;
    int64_t found = 0, stv[6] = {0, 0, 0, 0, 0, 0};
    st.run([&] {
        if (int r = cluster(s, radius, min_points, labels_d, sizes_d, core_d, counts_d, &found, stv)) return r;
        const hipError_t e = copy_out(sizes, sizes_d, (size_t)found);   // (the C clusters only: the rest of the caller's array stays)
        return e == hipSuccess ? SDFK_OK : fail(SDFK_ERR_HIP, "sdfk_points_cluster: %s", hipGetErrorString(e));
    });
    const int r = st.finish("sdfk_points_cluster");
    if (!r) {
        if (n_clusters) *n_clusters = found;
        if (stats)
            for (int i = 0; i < 6; i++) stats[i] = stv[i];
    }
    return r;
}

extern "C" int sdfk_points_select_device(const sdfk_points* s, const void* labels_dev, const void* keep_dev, int64_t n_clusters, void* index_out_dev,
                                         void* points_out_dev, int64_t* n_kept)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_select(s, labels_dev, keep_dev, n_clusters)) return r;
    return select(s, (const int32_t*)labels_dev, (const uint8_t*)keep_dev, n_clusters, (int32_t*)index_out_dev, (float*)points_out_dev, n_kept);
}

extern "C" int sdfk_points_select(const sdfk_points* s, const int32_t* labels, const uint8_t* keep, int64_t n_clusters, int32_t* index_out,
                                  float* points_out, int64_t* n_kept)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_select(s, labels, keep, n_clusters)) return r;
    const size_t n = (size_t)s->n;
    Staged st;
    const int32_t* labels_d = st.in(labels, n);
    const uint8_t* keep_d = st.in(keep, (size_t)n_clusters);
    int32_t* index_d = index_out ? st.scratch<int32_t>(n) : nullptr;
    float* points_d = points_out ? st.scratch<float>(n * 3) : nullptr;
    int64_t kept = 0;
    st.run([&] {
        if (int r = select(s, labels_d, keep_d, n_clusters, index_d, points_d, &kept)) return r;
        hipError_t e = copy_out(index_out, index_d, (size_t)kept);   // (the kept ones only)
        if (e == hipSuccess) e = copy_out(points_out, points_d, (size_t)kept * 3);
        return e == hipSuccess ? SDFK_OK : fail(SDFK_ERR_HIP, "sdfk_points_select: %s", hipGetErrorString(e));
    });
    const int r = st.finish("sdfk_points_select");
    if (!r && n_kept) *n_kept = kept;
    return r;
}
