// lib_trimesh_weld.hip -- sdfk_trimesh_weld*: the vertices of a handle's mesh grouped by position (exactly, or by the cell of a
// lattice), every group replaced by its lowest index, the triangles rewritten and the mesh renumbered.  Contract:
// include/sdfkit_hip.h, "Triangle meshes: welding".  Decisions: trimesh_weld.h (shared with a host test).  The handle:
// trimesh_handle.h; it is not changed and keeps nothing of this.  Every decision is made on integers; no float atomics; no kernel
// has a loop whose bound depends on the data.
//
//   k_tw_bounds    (lattice) the least and greatest coordinate per axis over all vertices, as ordered integers: every lane strides
//                  over the vertices (a bound that depends on nv alone), a wave reduction,
//                  then one atomicMin and one atomicMax per wave and axis -- only from a wave that moves the extreme, so that the
//                  one address is not hit by every wave.  The host makes the lattice from them, or refuses.
//   k_tw_keys      one 16-byte record (key, index = v) per vertex: the lattice key, or the first key of exact mode (x).  On the
//                  way the OR over all vertices of key ^ key[0] (exact mode: of both keys), per wave and then one atomic OR (only
//                  from a wave that brings a new bit): the bytes in which all keys agree need no pass.
//   radix sort     device_sort.h, over the passes left.  Exact mode sorts twice: k_tw_rekey gives every sorted record its second
//                  key (z above y) from its index, and the second stable sort keeps the order of the first among equals.
//   k_tw_heads     head flag of every sorted record (exact: the three canonical coordinates gathered through the indices of the
//                  record and its predecessor); one scan numbers the groups.
//   k_tw_first     a head writes its index to group_first[group].   k_tw_rep   rep[index] = group_first[group]: the sorts are
//                  stable from ascending indices, so the head is the lowest index of its group.
//   k_tw_tri_flags keep flag of every rewritten triangle; a kept one stores the byte 1 at its three representatives.
//   k_tw_vert_flags keep flag of every vertex; two scans.   k_tw_vertices / k_tw_triangles   vertex_map and the gathers.
// The steps up to rep are trimesh_groups (trimesh_handle.h), which lib_trimesh_simplify.hip starts from too.
// Host side: the scratch and the host form's device copies are held in a Staged (device_stage.h); the handle check
// (trimesh_check) and the launch size (grid1) are trimesh_handle.h's.
#include "lib_internal.h"
#include "device_scan.h"
#include "device_sort.h"
#include "trimesh_handle.h"
#include "trimesh_weld.h"

namespace {

using namespace sdfk_trimesh_wld;

constexpr int kBlock = 256;
constexpr unsigned kBoundsBlocks = 1024;   // of k_tw_bounds

typedef unsigned long long u64;

struct Ctl {
    uint32_t lo[3], hi[3];   // ordered bits
    u64 diff[2];             // the OR of key ^ key[0]: of the (first) sort, of exact mode's second sort
};

__device__ __forceinline__ u64 wave_or(u64 v)
{
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ void load3(const uint32_t* __restrict__ P, int64_t v, uint32_t p[3])
{
    p[0] = P[3 * v]; p[1] = P[3 * v + 1]; p[2] = P[3 * v + 2];
}

// ---- keys -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_tw_bounds(const uint32_t* __restrict__ P, int64_t nv, Ctl* ctl)
{
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    // (at most kBoundsBlocks blocks stride over the vertices: a lane sees vertices from all over the mesh, so the first waves
    // to finish already hold near-extremes and few later ones have to touch the six words)
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < nv; v += (int64_t)gridDim.x * kBlock) {
        uint32_t p[3];
        load3(P, v, p);
        for (int a = 0; a < 3; a++) {
            const uint32_t o = ordered_bits(p[a]);
            lo[a] = min(lo[a], o);
            hi[a] = max(hi[a], o);
        }
    }
    for (int a = 0; a < 3; a++) {
        const uint32_t l = wave_min(lo[a]), h = wave_max(hi[a]);
        // (a wave that cannot change the extreme does not touch it: the value only ever falls / rises, so what the relaxed load
        // sees is no nearer the end than the truth, and a stale one only costs an atomic that changes nothing)
        if ((threadIdx.x & 63) == 0) {
            if (l < __atomic_load_n(&ctl->lo[a], __ATOMIC_RELAXED)) atomicMin(&ctl->lo[a], l);
            if (h > __atomic_load_n(&ctl->hi[a], __ATOMIC_RELAXED)) atomicMax(&ctl->hi[a], h);
        }
    }
}

template <bool EXACT>
__global__ __launch_bounds__(kBlock) void k_tw_keys(const uint32_t* __restrict__ P, int64_t nv, Lattice L, Rec* __restrict__ rec, Ctl* ctl)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    u64 d0 = 0, d1 = 0;
    if (v < nv) {
        uint32_t p[3], p0[3];
        load3(P, v, p);
        load3(P, 0, p0);
        const u64 key = EXACT ? exact_key_first(p) : lattice_key(L, p);
        rec[v] = Rec{key, (uint32_t)v, 0u};
        d0 = key_diff(key, EXACT ? exact_key_first(p0) : lattice_key(L, p0));
        if (EXACT) d1 = key_diff(exact_key_second(p), exact_key_second(p0));
    }
    d0 = wave_or(d0);
    d1 = wave_or(d1);
    // (only a wave that brings a new bit adds it: bits are only ever set, so a stale load only costs an atomic that changes nothing)
    if ((threadIdx.x & 63) == 0) {
        if (d0 & ~__atomic_load_n(&ctl->diff[0], __ATOMIC_RELAXED)) atomicOr(&ctl->diff[0], d0);
        if (d1 & ~__atomic_load_n(&ctl->diff[1], __ATOMIC_RELAXED)) atomicOr(&ctl->diff[1], d1);
    }
}

__global__ __launch_bounds__(kBlock) void k_tw_rekey(const uint32_t* __restrict__ P, Rec* __restrict__ s, int64_t n)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    uint32_t p[3];
    load3(P, s[j].index, p);
    s[j].key = exact_key_second(p);
}

// ---- groups -----------------------------------------------------------------------------------------------------------------
template <bool EXACT>
__global__ __launch_bounds__(kBlock) void k_tw_heads(const uint32_t* __restrict__ P, const Rec* __restrict__ s, int64_t n, uint32_t* __restrict__ head)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    bool same = false;
    if (j > 0) {
        if (EXACT) {
            uint32_t p[3], q[3];
            load3(P, s[j].index, p);
            load3(P, s[j - 1].index, q);
            same = exact_same(p, q);
        } else {
            same = s[j].key == s[j - 1].key;
        }
    }
    head[j] = is_head(j, same) ? 1u : 0u;
}

// head: scanned (head[n] = the number of groups)
__global__ __launch_bounds__(kBlock) void k_tw_first(const Rec* __restrict__ s, int64_t n, const uint32_t* __restrict__ head, int32_t* __restrict__ group_first)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t g0 = head[j];
    if (head[j + 1] != g0 && g0 < n) group_first[g0] = (int32_t)s[j].index;   // (g0 < groups <= n)
}

// order (or null): the vertex of every sorted position, for a caller that walks the members of a group
__global__ __launch_bounds__(kBlock) void k_tw_rep(const Rec* __restrict__ s, int64_t n, const uint32_t* __restrict__ head,
                                                   const int32_t* __restrict__ group_first, int32_t* __restrict__ rep, uint32_t* __restrict__ order)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t g0 = head[j], grp = group_of(g0, head[j + 1] != g0);
    const uint32_t v = s[j].index;
    if (order) order[j] = v;
    if (grp < n && v < n) rep[v] = group_first[grp];   // (always: sorted position 0 is a head, and the indices are 0 .. n - 1)
}

// ---- what is kept -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_tw_tri_flags(const int32_t* __restrict__ idx, int64_t nt, const int32_t* __restrict__ rep, int32_t flags,
                                                         uint32_t* __restrict__ tflag, uint8_t* __restrict__ used)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const int32_t a = rep[idx[3 * t]], b = rep[idx[3 * t + 1]], c = rep[idx[3 * t + 2]];
    const bool keep = keeps_triangle(a, b, c, flags);
    tflag[t] = keep ? 1u : 0u;
    if (keep) { used[a] = 1; used[b] = 1; used[c] = 1; }   // (every writer stores the same byte)
}

__global__ __launch_bounds__(kBlock) void k_tw_vert_flags(const int32_t* __restrict__ rep, const uint8_t* __restrict__ used, int64_t nv, int32_t flags,
                                                          uint32_t* __restrict__ vflag)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    vflag[v] = keeps_vertex((int32_t)v, rep[v], used[v] != 0, flags) ? 1u : 0u;
}

struct WeldOut {
    int32_t* vertex_map;
    int32_t* vertex_index;
    int32_t* triangle_index;
    int32_t* triangles;
    float* vertices;
    float* colors;
};

// vnew: the scanned vertex flags (vnew[v + 1] != vnew[v]: v is kept, as vertex vnew[v])
__global__ __launch_bounds__(kBlock) void k_tw_vertices(const uint32_t* __restrict__ vnew, const int32_t* __restrict__ rep, int64_t nv,
                                                        const float* __restrict__ vertices, const float* __restrict__ colors, WeldOut O)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const int64_t r = rep[v];
    const int64_t o = vnew[r];
    const bool kept = vnew[r + 1] != o;
    if (O.vertex_map) O.vertex_map[v] = map_of(kept, (uint32_t)o);
    if (r != v || !kept || o >= nv) return;
    if (O.vertex_index) O.vertex_index[o] = (int32_t)v;
    for (int a = 0; a < 3; a++) {
        if (O.vertices) O.vertices[3 * o + a] = vertices[3 * v + a];
        if (O.colors) O.colors[3 * o + a] = colors ? colors[3 * v + a] : 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void k_tw_triangles(const uint32_t* __restrict__ tnew, int64_t nt, const uint32_t* __restrict__ vnew,
                                                         const int32_t* __restrict__ rep, const int32_t* __restrict__ idx, WeldOut O)
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
int check(const sdfk_trimesh* t, float tolerance, int32_t flags, const char* who)
{
    if (int r = trimesh_check(t, who, 0)) return r;   // (no records per triangle here: the sort is over the vertices)
    if (!tolerance_is_valid(tolerance)) return fail(SDFK_ERR_INVALID, "%s: tolerance must be finite and not negative", who);
    if (!flags_are_valid(flags)) return fail(SDFK_ERR_INVALID, "%s: unknown flag bits", who);
    return SDFK_OK;
}

}  // namespace

// The groups of the handle's vertices (trimesh_handle.h): the steps up to rep, queued on st; the lattice's box and the pass masks
// come back to the host on the way, so G->passes is final on return.
void trimesh_groups(const sdfk_trimesh* t, float tolerance, bool want_order, Staged& st, TrimeshGroups* G, const char* who)
{
    const int64_t nv = t->nv, n = nv;
    const bool exact = tolerance == 0.0f;
    const uint32_t* P = (const uint32_t*)t->vertices;
    Ctl* ctl = st.scratch<Ctl>(1);
    Rec* ra = st.scratch<Rec>((size_t)n);
    Rec* rb = st.scratch<Rec>((size_t)n);
    Rec* sorted = nullptr;
    uint32_t* head = st.scratch<uint32_t>((size_t)n + 1);
    int32_t* group_first = st.scratch<int32_t>((size_t)n);
    int32_t* rep = st.scratch<int32_t>((size_t)nv);
    uint32_t* order = want_order ? st.scratch<uint32_t>((size_t)n) : nullptr;
    Ctl host{{0xffffffffu, 0xffffffffu, 0xffffffffu}, {0u, 0u, 0u}, {0ull, 0ull}};
    Lattice L{};
    unsigned lattice_mask = 0xffu;
    int passes = 0;
    st.run([&] { return hipMemcpyAsync(ctl, &host, sizeof host, hipMemcpyHostToDevice, g.stream); });
    if (!exact) {
        st.run([&] {
            ProfScope ps("k_tw_bounds");
            hipLaunchKernelGGL(k_tw_bounds, dim3(std::min(grid1(nv), kBoundsBlocks)), dim3(kBlock), 0, g.stream, P, nv, ctl);
        });
        st.read(&host, ctl, sizeof host);
        st.run([&] {
            float lo[3], hi[3];
            for (int a = 0; a < 3; a++) {
                lo[a] = float_of(unordered_bits(host.lo[a]));
                hi[a] = float_of(unordered_bits(host.hi[a]));
            }
            if (!lattice_of(tolerance, lo, hi, &L, &lattice_mask)) return fail(SDFK_ERR_INVALID, "%s: an axis spans 2^21 cells of the tolerance or more", who);
            return (int)SDFK_OK;
        });
    }
    st.run([&] {
        ProfScope ps("k_tw_keys");
        if (exact) hipLaunchKernelGGL(k_tw_keys<true>, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, P, nv, L, ra, ctl);
        else hipLaunchKernelGGL(k_tw_keys<false>, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, P, nv, L, ra, ctl);
    });
    st.read(&host, ctl, sizeof host);
    st.run([&] {
        const unsigned mask = pass_mask(host.diff[0]) & lattice_mask;
        passes += passes_of(mask);
        return radix_sort(ra, rb, n, mask, &sorted, who);
    });
    if (const unsigned mask = exact ? pass_mask(host.diff[1]) : 0u) {
        st.run([&] {
            ProfScope ps("k_tw_rekey");
            hipLaunchKernelGGL(k_tw_rekey, dim3(grid1(n)), dim3(kBlock), 0, g.stream, P, sorted, n);
        });
        passes += passes_of(mask);
        st.run([&] { return radix_sort(sorted, sorted == ra ? rb : ra, n, mask, &sorted, who); });
    }
    {
        ProfScope ps("k_tw_groups");
        st.run([&] {
            if (exact) hipLaunchKernelGGL(k_tw_heads<true>, dim3(grid1(n)), dim3(kBlock), 0, g.stream, P, sorted, n, head);
            else hipLaunchKernelGGL(k_tw_heads<false>, dim3(grid1(n)), dim3(kBlock), 0, g.stream, P, sorted, n, head);
        });
        st.run([&] { return sdfk_scan::scan(head, n, who); });
        st.run([&] {
            hipLaunchKernelGGL(k_tw_first, dim3(grid1(n)), dim3(kBlock), 0, g.stream, sorted, n, head, group_first);
            hipLaunchKernelGGL(k_tw_rep, dim3(grid1(n)), dim3(kBlock), 0, g.stream, sorted, n, head, group_first, rep, order);
        });
    }
    *G = TrimeshGroups{order, head, group_first, rep, passes};
}

namespace {

// O: device buffers (any may be null); synchronises: the counts and stats are read on the way
int weld(const sdfk_trimesh* t, float tolerance, int32_t flags, WeldOut O, int64_t* nv_out, int64_t* nt_out, int64_t stats[4], const char* who)
{
    const int64_t nv = t->nv, nt = t->nt, n = nv;
    Staged st;
    TrimeshGroups G{};
    trimesh_groups(t, tolerance, false, st, &G, who);
    uint32_t* head = G.head;
    int32_t* rep = G.rep;
    uint8_t* used = st.scratch<uint8_t>((size_t)nv);
    uint32_t* vnew = st.scratch<uint32_t>((size_t)nv + 1);
    uint32_t* tnew = st.scratch<uint32_t>((size_t)nt + 1);
    uint32_t counts[3] = {0, 0, 0};   // groups, kept vertices, kept triangles
    st.run([&] { return hipMemsetAsync(used, 0, (size_t)nv, g.stream); });
    {
        ProfScope ps("k_tw_output");
        st.run([&] {
            hipLaunchKernelGGL(k_tw_tri_flags, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->idx, nt, rep, flags, tnew, used);
            hipLaunchKernelGGL(k_tw_vert_flags, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, rep, used, nv, flags, vnew);
        });
        st.run([&] { return sdfk_scan::scan(vnew, nv, who); });
        st.run([&] { return sdfk_scan::scan(tnew, nt, who); });
        st.run([&] {
            hipLaunchKernelGGL(k_tw_vertices, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, vnew, rep, nv, t->vertices, t->colors, O);
            hipLaunchKernelGGL(k_tw_triangles, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, tnew, nt, vnew, rep, t->idx, O);
        });
        st.run([&] { return hipMemcpyAsync(&counts[0], head + n, sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream); });
        st.run([&] { return hipMemcpyAsync(&counts[1], vnew + nv, sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream); });
        st.run([&] { return hipMemcpyAsync(&counts[2], tnew + nt, sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream); });
    }
    if (int r = st.finish(who)) return r;   // (synchronises: the counts are read)
    if (nv_out) *nv_out = counts[1];
    if (nt_out) *nt_out = counts[2];
    if (stats) {
        stats[kStatMerged] = nv - (int64_t)counts[0];
        stats[kStatDegenerate] = nt - (int64_t)counts[2];
        stats[kStatUnreferenced] = (int64_t)counts[0] - (int64_t)counts[1];
        stats[kStatPasses] = G.passes;
    }
    return SDFK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_trimesh_weld_device(sdfk_trimesh* t, float tolerance, int32_t flags, void* vertex_map_dev, void* vertex_index_out_dev,
                                        void* triangle_index_out_dev, void* triangles_out_dev, void* vertices_out_dev, void* colors_out_dev,
                                        int64_t* nv_out, int64_t* nt_out, int64_t stats[4])
{
    static const char* who = "sdfk_trimesh_weld";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check(t, tolerance, flags, who)) return r;
    return weld(t, tolerance, flags,
                WeldOut{(int32_t*)vertex_map_dev, (int32_t*)vertex_index_out_dev, (int32_t*)triangle_index_out_dev, (int32_t*)triangles_out_dev,
                        (float*)vertices_out_dev, (float*)colors_out_dev},
                nv_out, nt_out, stats, who);
}

extern "C" int sdfk_trimesh_weld(sdfk_trimesh* t, float tolerance, int32_t flags, int32_t* vertex_map, int32_t* vertex_index_out,
                                 int32_t* triangle_index_out, int32_t* triangles_out, float* vertices_out, float* colors_out, int64_t* nv_out,
                                 int64_t* nt_out, int64_t stats[4])
{
    static const char* who = "sdfk_trimesh_weld";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check(t, tolerance, flags, who)) return r;
    const size_t nv = (size_t)t->nv, nt = (size_t)t->nt;
    Staged st;
    const WeldOut O{st.out(vertex_map, nv), vertex_index_out ? st.scratch<int32_t>(nv) : nullptr,
                    triangle_index_out ? st.scratch<int32_t>(nt) : nullptr, triangles_out ? st.scratch<int32_t>(3 * nt) : nullptr,
                    vertices_out ? st.scratch<float>(3 * nv) : nullptr, colors_out ? st.scratch<float>(3 * nv) : nullptr};
    int64_t kv = 0, kt = 0, stv[4] = {0, 0, 0, 0};
    st.run([&] { return weld(t, tolerance, flags, O, &kv, &kt, stv, who); });   // (synchronises: the counts size the copies back)
    st.run([&] { return copy_out(vertex_index_out, O.vertex_index, (size_t)kv); });   // (the kept ones only: the rest of the caller's arrays stays)
    st.run([&] { return copy_out(triangle_index_out, O.triangle_index, (size_t)kt); });
    st.run([&] { return copy_out(triangles_out, O.triangles, 3 * (size_t)kt); });
    st.run([&] { return copy_out(vertices_out, O.vertices, 3 * (size_t)kv); });
    st.run([&] { return copy_out(colors_out, O.colors, 3 * (size_t)kv); });
    if (int r = st.finish(who)) return r;
    if (nv_out) *nv_out = kv;
    if (nt_out) *nt_out = kt;
    if (stats)
        for (int k = 0; k < 4; k++) stats[k] = stv[k];
    return SDFK_OK;
}
