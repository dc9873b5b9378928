// lib_trimesh_topology.hip -- the connectivity of a triangle mesh by index: sdfk_trimesh_components* (a label per vertex and per
// triangle), sdfk_trimesh_topology* (the edge census, a row per component) and sdfk_trimesh_select* (the sub-mesh of the kept
// components, renumbered).  Contract: include/sdfkit_hip.h, "Triangle meshes: topology".  Decisions: trimesh_topology.h (shared
// with a host test).  The handle: trimesh_handle.h.  Everything accumulated is an integer; no float atomics; no kernel has a loop
// whose bound depends on the data.
//
// Labels (once per handle):
//   k_tt_init      parent[v] = v, referenced[v] = 0.          k_tt_ref   referenced[corner] = 1 for every connecting triangle.
//   k_tt_hook      one lane per triangle: the least parent of its corners goes, by atomicMin, to the parents of the other corners'
//                  parents; changes are counted.  Labels only decrease and always name a vertex of the same component.
//   k_tt_shortcut  one lane per vertex: parent[v] = parent[parent[v]], one jump per launch; changes are counted.  A launch that
//                  finds that the launch before it changed nothing returns at once: the forest is flat.
//                  The host queues a hook round and kShortcuts shortcut launches, reads the counters once, queues more shortcut
//                  launches while the last one still changed something, and ends when a hook round on a flat forest changed
//                  nothing.  Every verdict is read from a counter that the launch BEFORE the reader finished: no launch relies on
//                  seeing another workgroup's writes, a stale read only costs a round.
//   k_tt_roots     root flags; a scan numbers them (ascending root).  k_tt_vlabel / k_tt_tlabel write the labels.
// Census (per call):
//   k_tt_keys      three (key, triangle, forward) records per triangle; an index-degenerate triangle writes the skip key.
//   radix sort     device_sort.h, over the bytes of each half of the key that nv can set.
//   k_tt_heads     head flag and forward bit of every sorted position; two scans.   k_tt_starts  the start of every run.
//   k_tt_edges     one lane per run head: m and f from the starts and the scanned forward bits, the class, the adds.
//   k_tt_tri_rows / k_tt_vert_rows   triangles, area weights and vertices per component.
//   Every add is summed over the wave first: one atomic per wave and column into the census, and, where the wave's lanes all
//   name one component (always, on a single-component mesh), one into its row; only a mixed wave adds lane by lane.
// Select:
//   k_ts_flags     keep flags per vertex and per triangle; two scans.   k_ts_vertices / k_ts_triangles   the gathers.
// Host side: scratch, adopted labels and the host forms' device copies are held in a Staged (device_stage.h); the handle check
// (trimesh_check) and the launch size (grid1) are trimesh_handle.h's.
#include "lib_internal.h"
#include "device_scan.h"
#include "device_sort.h"
#include "device_wave.h"
#include "trimesh_handle.h"
#include "trimesh_topology.h"

namespace {

using namespace sdfk_trimesh_topo;

constexpr int kBlock = 256;
constexpr int kShortcuts = 8;        // shortcut launches queued per read of the counters
constexpr int kMaxShortcutBatches = 8;   // per hook round: 64 jumps flatten any tree of fewer than 2^31 vertices (depth halves per jump)

typedef unsigned long long u64;

struct Ctl {
    unsigned count[3];     // changes of launch q in slot q % 3
    unsigned pad;
    u64 hook_changes;      // over all hook rounds
    u64 rounds, shortcuts; // hook rounds run, shortcut launches that worked
};

// ---- labels -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_tt_init(int32_t* __restrict__ parent, uint8_t* __restrict__ referenced, int64_t nv)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    parent[v] = (int32_t)v;
    referenced[v] = 0;
}

__global__ __launch_bounds__(kBlock) void k_tt_ref(const int32_t* __restrict__ idx, int64_t nt, uint8_t* __restrict__ referenced)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const int32_t a = idx[3 * t], b = idx[3 * t + 1], c = idx[3 * t + 2];
    if (index_degenerate(a, b, c)) return;
    referenced[a] = 1; referenced[b] = 1; referenced[c] = 1;   // (every writer stores the same byte)
}

__global__ __launch_bounds__(kBlock) void k_tt_hook(const int32_t* __restrict__ idx, int64_t nt, int32_t* parent, Ctl* ctl, int q)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->count[(q + 1) % 3] = 0;
        ctl->rounds += 1;
    }
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned changed = 0;
    if (t < nt) {
        const int32_t a = idx[3 * t], b = idx[3 * t + 1], c = idx[3 * t + 2];
        if (!index_degenerate(a, b, c)) {
            const int32_t p[3] = {__atomic_load_n(&parent[a], __ATOMIC_RELAXED), __atomic_load_n(&parent[b], __ATOMIC_RELAXED),
                                  __atomic_load_n(&parent[c], __ATOMIC_RELAXED)};
            const int32_t m = hook_target(p[0], p[1], p[2]);
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (p[k] != m && hook_changes(atomicMin(&parent[p[k]], m), m)) changed++;
        }
    }
    const u64 n = wave_sum(changed);
    if ((threadIdx.x & 63) == 0 && n) {
        atomicAdd(&ctl->count[q % 3], (unsigned)n);
        atomicAdd(&ctl->hook_changes, n);
    }
}

__global__ __launch_bounds__(kBlock) void k_tt_shortcut(int32_t* parent, int64_t nv, Ctl* ctl, int q)
{
    const unsigned before = ctl->count[(q + 2) % 3];   // (of the launch before this one: complete)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->count[(q + 1) % 3] = 0;
        if (before) ctl->shortcuts += 1;
    }
    if (!before) return;   // flat already: this launch's own count stays 0
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned changed = 0;
    if (v < nv) {
        const int32_t p = __atomic_load_n(&parent[v], __ATOMIC_RELAXED);
        const int32_t gp = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
        if (gp < p) {
            __atomic_store_n(&parent[v], gp, __ATOMIC_RELAXED);
            changed = 1;
        }
    }
    const u64 n = wave_sum(changed);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&ctl->count[q % 3], (unsigned)n);
}

__global__ __launch_bounds__(kBlock) void k_tt_roots(const int32_t* __restrict__ parent, const uint8_t* __restrict__ referenced, int64_t nv,
                                                     uint32_t* __restrict__ flag)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    flag[v] = is_root((int32_t)v, parent[v], referenced[v] != 0) ? 1u : 0u;
}

// number: the scanned root flags (number[r] of a root r = its component)
__global__ __launch_bounds__(kBlock) void k_tt_vlabel(const int32_t* __restrict__ parent, const uint8_t* __restrict__ referenced, int64_t nv,
                                                      const uint32_t* __restrict__ number, int32_t* __restrict__ label)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    label[v] = referenced[v] ? (int32_t)number[parent[v]] : -1;
}

__global__ __launch_bounds__(kBlock) void k_tt_tlabel(const int32_t* __restrict__ idx, int64_t nt, const int32_t* __restrict__ vlabel,
                                                      int32_t* __restrict__ label)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const int32_t a = idx[3 * t], b = idx[3 * t + 1], c = idx[3 * t + 2];
    label[t] = index_degenerate(a, b, c) ? -1 : vlabel[a];
}

// ---- the rows ---------------------------------------------------------------------------------------------------------------
// Every lane of the wave comes here.  c: the lane's component, -1: nothing to add.  -> whether the lanes that add all name one
// component (*c0), so that lane 0 may add the wave's sums to that row.
__device__ __forceinline__ bool wave_uniform(int32_t c, int32_t* c0)
{
    const u64 valid = __ballot(c >= 0);
    *c0 = -1;
    if (!valid) return false;
    *c0 = __shfl(c, __ffsll((long long)valid) - 1);
    return __ballot(c >= 0 && c != *c0) == 0;
}

__global__ __launch_bounds__(kBlock) void k_tt_tri_rows(const int32_t* __restrict__ tlabel, const u64* __restrict__ W, int64_t nt, u64* rows)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int32_t c = t < nt ? tlabel[t] : -1;
    const u64 w = c >= 0 ? W[t + 1] - W[t] : 0ull;
    int32_t c0;
    const bool uniform = wave_uniform(c, &c0);   // (no census column: the triangles of the mesh are nt less the degenerate ones)
    if (c0 < 0) return;
    if (uniform) {
        const u64 n = wave_sum(c >= 0 ? 1ull : 0ull), ws = wave_sum(w);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&rows[(size_t)c0 * kRow + kTriangles], n);
            if (ws) atomicAdd(&rows[(size_t)c0 * kRow + kAreaWeight], ws);
        }
    } else if (c >= 0) {
        atomicAdd(&rows[(size_t)c * kRow + kTriangles], 1ull);
        if (w) atomicAdd(&rows[(size_t)c * kRow + kAreaWeight], w);
    }
}

__global__ __launch_bounds__(kBlock) void k_tt_vert_rows(const int32_t* __restrict__ vlabel, int64_t nv, u64* rows, u64* census)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int32_t c = v < nv ? vlabel[v] : -1;
    int32_t c0;
    const bool uniform = wave_uniform(c, &c0);
    if (c0 < 0) return;
    const u64 n = wave_sum(c >= 0 ? 1ull : 0ull);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&census[kCensusVertices], n);
        if (uniform) atomicAdd(&rows[(size_t)c0 * kRow + kVertices], n);
    }
    if (!uniform && c >= 0) atomicAdd(&rows[(size_t)c * kRow + kVertices], 1ull);
}

// ---- the edge census --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_tt_keys(const int32_t* __restrict__ idx, int64_t nt, Rec* __restrict__ rec, u64* census)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    u64 degenerate = 0;
    if (t < nt) {
        const int32_t tri[3] = {idx[3 * t], idx[3 * t + 1], idx[3 * t + 2]};
        const bool skip = index_degenerate(tri[0], tri[1], tri[2]);
        degenerate = skip ? 1ull : 0ull;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            int32_t u, v;
            directed_edge(tri, k, &u, &v);
            rec[3 * t + k] = skip ? Rec{kSkipKey, (uint32_t)t, 0u} : Rec{edge_key(u, v), (uint32_t)t, edge_forward(u, v) ? 1u : 0u};
        }
    }
    wave_add(&census[kCensusDegenerate], degenerate);
}

__global__ __launch_bounds__(kBlock) void k_tt_heads(const Rec* __restrict__ s, int64_t n, uint32_t* __restrict__ head, uint32_t* __restrict__ fwd)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    head[j] = (j == 0 || s[j].key != s[j - 1].key) ? 1u : 0u;
    fwd[j] = s[j].pad;
}

// head: scanned (head[n] = the number of runs).  start[r] = the sorted position run r begins at, start[runs] = n.
__global__ __launch_bounds__(kBlock) void k_tt_starts(const Rec* __restrict__ s, int64_t n, const uint32_t* __restrict__ head, uint32_t* __restrict__ start)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    if (j == 0 || s[j].key != s[j - 1].key) start[head[j]] = (uint32_t)j;   // (head[j] < runs <= n)
    if (j == 0) start[head[n]] = (uint32_t)n;
}

__global__ __launch_bounds__(kBlock) void k_tt_edges(const Rec* __restrict__ s, int64_t n, const uint32_t* __restrict__ head,
                                                     const uint32_t* __restrict__ fwd, const uint32_t* __restrict__ start,
                                                     const int32_t* __restrict__ vlabel, u64* rows, u64* census)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t c = -1;
    u64 packed = 0;
    if (j < n) {
        const uint64_t key = s[j].key;
        if (key != kSkipKey && (j == 0 || key != s[j - 1].key)) {
            const uint32_t end = start[head[j] + 1];
            if (end > (uint32_t)j && end <= n) {   // (always)
                packed = edge_packed(edge_class(end - (uint32_t)j, fwd[end] - fwd[j]));
                c = vlabel[edge_low_vertex(key)];
            }
        }
    }
    int32_t c0;
    const bool uniform = wave_uniform(c, &c0);
    if (c0 < 0) return;
    const u64 sum = wave_sum(c >= 0 ? packed : 0ull);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 5; k++) {
            const u64 v = packed_byte(sum, k);
            if (!v) continue;
            atomicAdd(&census[kCensusEdges + k], v);
            if (uniform) atomicAdd(&rows[(size_t)c0 * kRow + kEdges + k], v);
        }
    if (!uniform && c >= 0)
        for (int k = 0; k < 5; k++)
            if (packed_byte(packed, k)) atomicAdd(&rows[(size_t)c * kRow + kEdges + k], 1ull);
}

// ---- select -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ts_flags(const int32_t* __restrict__ label, int64_t n, const uint8_t* __restrict__ keep,
                                                     uint32_t* __restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    flag[i] = keeps(label[i], keep) ? 1u : 0u;
}

// vnew: the scanned vertex flags (vnew[v + 1] != vnew[v]: v is kept, as vertex vnew[v])
__global__ __launch_bounds__(kBlock) void k_ts_vertices(const uint32_t* __restrict__ vnew, int64_t nv, const float* __restrict__ vertices,
                                                        const float* __restrict__ colors, int32_t* __restrict__ index_out,
                                                        float* __restrict__ vertices_out, float* __restrict__ colors_out)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const int64_t o = vnew[v];
    if (vnew[v + 1] == o || o >= nv) return;
    if (index_out) index_out[o] = (int32_t)v;
    for (int a = 0; a < 3; a++) {
        if (vertices_out) vertices_out[3 * o + a] = vertices[3 * v + a];
        if (colors_out) colors_out[3 * o + a] = colors ? colors[3 * v + a] : 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void k_ts_triangles(const uint32_t* __restrict__ tnew, int64_t nt, const uint32_t* __restrict__ vnew,
                                                         const int32_t* __restrict__ idx, int32_t* __restrict__ index_out,
                                                         int32_t* __restrict__ triangles_out)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const int64_t o = tnew[t];
    if (tnew[t + 1] == o || o >= nt) return;
    if (index_out) index_out[o] = (int32_t)t;
    if (triangles_out)
        for (int k = 0; k < 3; k++) triangles_out[3 * o + k] = (int32_t)vnew[idx[3 * t + k]];   // (a kept triangle's corners are kept)
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// The labels, once per handle: synchronises (the rounds end on a counter the host reads).
int labels_prepare(sdfk_trimesh* t, const char* who)
{
    if (t->comp_vertex) return SDFK_OK;
    const int64_t nv = t->nv, nt = t->nt;
    Staged st;
    int32_t* parent = st.scratch<int32_t>((size_t)nv);
    uint8_t* referenced = st.scratch<uint8_t>((size_t)nv);
    uint32_t* flag = st.scratch<uint32_t>((size_t)nv + 1);
    Ctl* ctl = st.scratch<Ctl>(1);
    int32_t* vlabel = st.kept<int32_t>((size_t)nv);
    int32_t* tlabel = st.kept<int32_t>((size_t)nt);
    Ctl host{};
    uint32_t count = 0;
    st.run([&] { return hipMemsetAsync(ctl, 0, sizeof(Ctl), g.stream); });
    st.run([&] {
        ProfScope ps("k_tt_init");
        hipLaunchKernelGGL(k_tt_init, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, parent, referenced, nv);
        hipLaunchKernelGGL(k_tt_ref, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->idx, nt, referenced);
    });
    int q = 0;   // launches numbered so far (only q % 3 is used)
    bool flat = true;
    int batches = 0;
    u64 hook_before = 0;
    while (st.ok()) {
        if (flat) {
            if ((int64_t)host.rounds >= max_rounds(nv)) {
                st.run([&] { return fail(SDFK_ERR_INVALID, "%s: the label rounds did not end within n_vertices + 1", who); });
                break;
            }
            hook_before = host.hook_changes;
            batches = 0;
            ProfScope ps("k_tt_hook");
            q = (q + 1) % 3;
            hipLaunchKernelGGL(k_tt_hook, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->idx, nt, parent, ctl, q);   // (its error: taken below)
        } else if (++batches > kMaxShortcutBatches) {
            st.run([&] { return fail(SDFK_ERR_INVALID, "%s: the shortcut launches did not flatten the labels", who); });
            break;
        }
        st.run([&] {
            ProfScope ps("k_tt_shortcut");
            for (int b = 0; b < kShortcuts; b++) {
                q = (q + 1) % 3;
                hipLaunchKernelGGL(k_tt_shortcut, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, parent, nv, ctl, q);
            }
        });
        st.read(&host, ctl, sizeof host);
        if (!st.ok()) break;
        flat = host.count[q] == 0;                                // the last shortcut launch changed nothing
        if (flat && host.hook_changes == hook_before) break;      // and the hook round before them, on a flat forest, neither
    }
    {
        ProfScope ps("k_tt_labels");
        st.run([&] { hipLaunchKernelGGL(k_tt_roots, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, parent, referenced, nv, flag); });
        st.run([&] { return sdfk_scan::scan(flag, nv, who); });
        st.run([&] {
            hipLaunchKernelGGL(k_tt_vlabel, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, parent, referenced, nv, flag, vlabel);
            hipLaunchKernelGGL(k_tt_tlabel, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->idx, nt, vlabel, tlabel);
        });
        st.read(&count, flag + nv, sizeof count);
    }
    if (int r = st.finish(who, false)) return r;   // (the read above has waited; the labels are the handle's from here)
    t->comp_vertex = vlabel;
    t->comp_triangle = tlabel;
    t->comp_count = (int64_t)count;
    t->comp_rounds = (int64_t)host.rounds;
    t->comp_shortcuts = (int64_t)host.shortcuts;
    return SDFK_OK;
}

// census8 (host) and the rows of the first min(C, capacity) components into rows_out (device memory, or host memory)
int topology(sdfk_trimesh* t, int64_t census8[8], int64_t* rows_out, int64_t capacity, bool device, const char* who)
{
    if (int r = labels_prepare(t, who)) return r;
    if (int r = trimesh_weights(t, who)) return r;
    const int64_t nv = t->nv, nt = t->nt, n = 3 * nt, C = t->comp_count;
    const size_t nrow = (size_t)(C + 1) * kRow;
    Staged st;
    u64* rows = st.scratch<u64>(nrow);     // C x 8, then the census
    Rec* ra = st.scratch<Rec>((size_t)n);
    Rec* rb = st.scratch<Rec>((size_t)n);
    Rec* sorted = nullptr;
    uint32_t* head = st.scratch<uint32_t>((size_t)n + 1);
    uint32_t* fwd = st.scratch<uint32_t>((size_t)n + 1);
    uint32_t* start = st.scratch<uint32_t>((size_t)n + 1);
    u64* census = rows ? rows + (size_t)C * kRow : nullptr;
    st.run([&] { return hipMemsetAsync(rows, 0, nrow * sizeof(u64), g.stream); });
    st.run([&] {
        ProfScope ps("k_tt_rows");
        hipLaunchKernelGGL(k_tt_tri_rows, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->comp_triangle, t->sample_W, nt, rows);
        hipLaunchKernelGGL(k_tt_vert_rows, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, t->comp_vertex, nv, rows, census);
        hipLaunchKernelGGL(k_tt_keys, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->idx, nt, ra, census);
    });
    st.run([&] { return radix_sort(ra, rb, n, key_digit_mask(nv), &sorted, who); });
    {
        ProfScope ps("k_tt_edges");
        st.run([&] { hipLaunchKernelGGL(k_tt_heads, dim3(grid1(n)), dim3(kBlock), 0, g.stream, sorted, n, head, fwd); });
        st.run([&] { return sdfk_scan::scan(head, n, who); });
        st.run([&] { return sdfk_scan::scan(fwd, n, who); });
        st.run([&] {
            hipLaunchKernelGGL(k_tt_starts, dim3(grid1(n)), dim3(kBlock), 0, g.stream, sorted, n, head, start);
            hipLaunchKernelGGL(k_tt_edges, dim3(grid1(n)), dim3(kBlock), 0, g.stream, sorted, n, head, fwd, start, t->comp_vertex, rows, census);
        });
    }
    u64 hc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t nout = std::min<int64_t>(C, capacity);
    if (rows_out && nout > 0)
        st.run([&] {
            return hipMemcpyAsync(rows_out, rows, (size_t)nout * kRow * sizeof(u64), device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, g.stream);
        });
    st.read(hc, census, sizeof hc);   // (synchronises: host rows have arrived, too)
    if (int r = st.finish(who, false)) return r;
    if (census8) {
        for (int k = 0; k < 8; k++) census8[k] = (int64_t)hc[k];
        census8[kCensusComponents] = C;
    }
    return SDFK_OK;
}

struct SelectOut {
    int32_t* vertex_index;
    int32_t* triangle_index;
    int32_t* triangles;
    float* vertices;
    float* colors;
};

// keep: C bytes of device memory; O: device buffers (any may be null); the counts are read on the way
int select_kept(sdfk_trimesh* t, const uint8_t* keep, SelectOut O, int64_t* nv_out, int64_t* nt_out, const char* who)
{
    const int64_t nv = t->nv, nt = t->nt;
    Staged st;
    uint32_t* vnew = st.scratch<uint32_t>((size_t)nv + 1);
    uint32_t* tnew = st.scratch<uint32_t>((size_t)nt + 1);
    uint32_t counts[2] = {0, 0};
    {
        ProfScope ps("k_ts_select");
        st.run([&] {
            hipLaunchKernelGGL(k_ts_flags, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, t->comp_vertex, nv, keep, vnew);
            hipLaunchKernelGGL(k_ts_flags, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->comp_triangle, nt, keep, tnew);
        });
        st.run([&] { return sdfk_scan::scan(vnew, nv, who); });
        st.run([&] { return sdfk_scan::scan(tnew, nt, who); });
        st.run([&] {
            hipLaunchKernelGGL(k_ts_vertices, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, vnew, nv, t->vertices, t->colors, O.vertex_index, O.vertices,
                               O.colors);
            hipLaunchKernelGGL(k_ts_triangles, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, tnew, nt, vnew, t->idx, O.triangle_index, O.triangles);
        });
        st.run([&] { return hipMemcpyAsync(&counts[0], vnew + nv, sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream); });
        st.run([&] { return hipMemcpyAsync(&counts[1], tnew + nt, sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream); });
    }
    if (int r = st.finish(who)) return r;   // (synchronises: the counts are read)
    if (nv_out) *nv_out = counts[0];
    if (nt_out) *nt_out = counts[1];
    return SDFK_OK;
}

void components_stats(const sdfk_trimesh* t, int64_t* n_components, int64_t stats[4])
{
    if (n_components) *n_components = t->comp_count;
    if (stats) {
        stats[0] = t->comp_rounds;
        stats[1] = t->comp_shortcuts;
        stats[2] = stats[3] = 0;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_trimesh_components_device(sdfk_trimesh* t, void* vertex_component_dev, void* triangle_component_dev, int64_t* n_components,
                                              int64_t stats[4])
{
    static const char* who = "sdfk_trimesh_components";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = trimesh_check(t, who, 3)) return r;
    if (int r = labels_prepare(t, who)) return r;
    // (written out, not Staged: two copies between device arrays that nothing here owns, and nothing to wait for)
    hipError_t e = hipSuccess;
    if (vertex_component_dev) e = hipMemcpyAsync(vertex_component_dev, t->comp_vertex, (size_t)t->nv * sizeof(int32_t), hipMemcpyDeviceToDevice, g.stream);
    if (e == hipSuccess && triangle_component_dev)
        e = hipMemcpyAsync(triangle_component_dev, t->comp_triangle, (size_t)t->nt * sizeof(int32_t), hipMemcpyDeviceToDevice, g.stream);
    if (e != hipSuccess) return fail(SDFK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    components_stats(t, n_components, stats);
    return SDFK_OK;
}

extern "C" int sdfk_trimesh_components(sdfk_trimesh* t, int32_t* vertex_component, int32_t* triangle_component, int64_t* n_components, int64_t stats[4])
{
    static const char* who = "sdfk_trimesh_components";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = trimesh_check(t, who, 3)) return r;
    if (int r = labels_prepare(t, who)) return r;
    Staged st;   // (no device copies: the labels are the handle's, and go straight into the caller's arrays)
    st.run([&] { return copy_out(vertex_component, t->comp_vertex, (size_t)t->nv); });
    st.run([&] { return copy_out(triangle_component, t->comp_triangle, (size_t)t->nt); });
    if (int r = st.finish(who)) return r;
    components_stats(t, n_components, stats);
    return SDFK_OK;
}

extern "C" int sdfk_trimesh_topology_device(sdfk_trimesh* t, int64_t census[8], void* component_rows_dev, int64_t capacity)
{
    static const char* who = "sdfk_trimesh_topology";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = trimesh_check(t, who, 3)) return r;
    if (capacity < 0) return fail(SDFK_ERR_INVALID, "%s: negative capacity", who);
    return topology(t, census, (int64_t*)component_rows_dev, capacity, true, who);
}

extern "C" int sdfk_trimesh_topology(sdfk_trimesh* t, int64_t census[8], int64_t* component_rows, int64_t capacity)
{
    static const char* who = "sdfk_trimesh_topology";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = trimesh_check(t, who, 3)) return r;
    if (capacity < 0) return fail(SDFK_ERR_INVALID, "%s: negative capacity", who);
    return topology(t, census, component_rows, capacity, false, who);
}

extern "C" int sdfk_trimesh_select_device(sdfk_trimesh* t, const void* keep_component_dev, void* vertex_index_out_dev, void* triangle_index_out_dev,
                                          void* triangles_out_dev, void* vertices_out_dev, void* colors_out_dev, int64_t* nv_out, int64_t* nt_out)
{
    static const char* who = "sdfk_trimesh_select";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = trimesh_check(t, who, 3)) return r;
    if (!keep_component_dev) return fail(SDFK_ERR_INVALID, "%s: null keep_component", who);
    if (int r = labels_prepare(t, who)) return r;
    return select_kept(t, (const uint8_t*)keep_component_dev,
                  SelectOut{(int32_t*)vertex_index_out_dev, (int32_t*)triangle_index_out_dev, (int32_t*)triangles_out_dev, (float*)vertices_out_dev,
                            (float*)colors_out_dev},
                  nv_out, nt_out, who);
}

extern "C" int sdfk_trimesh_select(sdfk_trimesh* t, const uint8_t* keep_component, int32_t* vertex_index_out, int32_t* triangle_index_out,
                                   int32_t* triangles_out, float* vertices_out, float* colors_out, int64_t* nv_out, int64_t* nt_out)
{
    static const char* who = "sdfk_trimesh_select";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = trimesh_check(t, who, 3)) return r;
    if (!keep_component) return fail(SDFK_ERR_INVALID, "%s: null keep_component", who);
    if (int r = labels_prepare(t, who)) return r;
    const size_t nv = (size_t)t->nv, nt = (size_t)t->nt, C = (size_t)t->comp_count;
    Staged st;
    uint8_t* keep = st.scratch<uint8_t>(std::max<size_t>(C, 1));
    if (C) st.run([&] { return hipMemcpyAsync(keep, keep_component, C, hipMemcpyHostToDevice, g.stream); });
    const SelectOut O{vertex_index_out ? st.scratch<int32_t>(nv) : nullptr, triangle_index_out ? st.scratch<int32_t>(nt) : nullptr,
                      triangles_out ? st.scratch<int32_t>(3 * nt) : nullptr, vertices_out ? st.scratch<float>(3 * nv) : nullptr,
                      colors_out ? st.scratch<float>(3 * nv) : nullptr};
    int64_t kv = 0, kt = 0;
    st.run([&] { return select_kept(t, keep, O, &kv, &kt, who); });   // (synchronises: the counts size the copies back)
    st.run([&] { return copy_out(vertex_index_out, O.vertex_index, (size_t)kv); });   // (the kept ones only: the rest of the caller's arrays stays)
    st.run([&] { return copy_out(triangle_index_out, O.triangle_index, (size_t)kt); });
    st.run([&] { return copy_out(triangles_out, O.triangles, 3 * (size_t)kt); });
    st.run([&] { return copy_out(vertices_out, O.vertices, 3 * (size_t)kv); });
    st.run([&] { return copy_out(colors_out, O.colors, 3 * (size_t)kv); });
    if (int r = st.finish(who)) return r;
    if (nv_out) *nv_out = kv;
    if (nt_out) *nt_out = kt;
    return SDFK_OK;
}
