// lib_trimesh_smooth.hip -- per-vertex gathers over the incidence of a triangle mesh: sdfk_trimesh_adjacency* (the neighbours of
// every vertex in compressed sparse rows, and the boundary bytes), sdfk_trimesh_smooth* (Laplacian / Taubin smoothing of the
// positions) and sdfk_trimesh_vertex_normals* (area-weighted normals from the geometry).  Contract: include/sdfkit_hip.h,
// "Triangle meshes: adjacency, smoothing, vertex normals".  Arithmetic and decisions: trimesh_adjacency.h (shared with a host
// test).  The handle: trimesh_handle.h.  No atomics but the sort's LDS counters; every sum runs in a stated order inside one lane;
// the boundary bytes are plain stores of the value 1.  No kernel has a loop whose bound depends on anything but its vertex's own
// degree (k_tv_step: its neighbours, k_tv_normals: its corners).
//
// The two structures (each once per handle, by the first call that needs it):
//   k_ta_nbr_keys / k_ta_corner_keys   six directed records / three corner records per triangle, in (t, k) order; an
//                  index-degenerate triangle writes records of the vertex nv, which sort behind everything.
//   radix sort     device_sort.h (stable), over the key bytes nv can set.
//   k_ta_heads     (neighbours) the head flag of every sorted position: a record of a vertex whose key differs from the one
//                  before; one scan numbers the entries, and its total sizes nbr.
//   k_ta_entries   one lane per sorted position: an entry writes its value (the neighbour / the corner) to its place; the first
//                  record of a vertex writes the vertex's first place; a run of one record sets both endpoints' boundary bytes.
//   k_ta_degree    the last record of a vertex writes the vertex's degree (its last place + 1 - its first place) over a zeroed
//                  array; one scan turns the degrees into nbr_start / inc_start.
// Smoothing: k_tv_step, one lane per vertex, one launch per step, ping-pong between the output and one temporary so that the
// last step writes the output; nothing waits on the host between the launches.
// Normals: k_tv_normals, one lane per vertex over its corners; the triangles' positions are gathered through the index array.
// Host side: scratch, the adopted structures and the host forms' device copies are held in a Staged (device_stage.h); the handle
// check (trimesh_check) and the launch size (grid1) are trimesh_handle.h's.
#include "lib_internal.h"
#include "device_scan.h"
#include "device_sort.h"
#include "trimesh_adjacency.h"
#include "trimesh_handle.h"

#include <cmath>

namespace {

using namespace sdfk_trimesh_adj;

constexpr int kBlock = 256;

// ---- the records ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ta_nbr_keys(const int32_t* __restrict__ idx, int64_t nt, int64_t nv, Rec* __restrict__ rec)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const int32_t tri[3] = {idx[3 * t], idx[3 * t + 1], idx[3 * t + 2]};
    const bool skip = index_degenerate(tri[0], tri[1], tri[2]);
#pragma unroll
    for (int j = 0; j < 6; j++) {
        int32_t from, to;
        directed_record(tri, j, &from, &to);
        rec[6 * t + j] = Rec{skip ? nbr_skip_key(nv) : nbr_key(from, to), (uint32_t)t, 0u};
    }
}

__global__ __launch_bounds__(kBlock) void k_ta_corner_keys(const int32_t* __restrict__ idx, int64_t nt, int64_t nv, Rec* __restrict__ rec)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const int32_t tri[3] = {idx[3 * t], idx[3 * t + 1], idx[3 * t + 2]};
    const bool skip = index_degenerate(tri[0], tri[1], tri[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) rec[3 * t + k] = Rec{skip ? corner_skip_key(nv) : (uint64_t)tri[k], (uint32_t)(3 * t + k), 0u};
}

__global__ __launch_bounds__(kBlock) void k_ta_heads(const Rec* __restrict__ s, int64_t n, int64_t nv, uint32_t* __restrict__ head)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    head[j] = entry_head(s[j].key, j > 0, j > 0 ? s[j - 1].key : 0ull, nv, 32) ? 1u : 0u;
}

// kShift = 32: the neighbours (place: the scanned head flags; value: `to`).  kShift = 0: the corners (every record of a vertex is
// an entry, at its own sorted position; value: the corner).  capacity: the length of `out`.
template <int kShift>
__global__ __launch_bounds__(kBlock) void k_ta_entries(const Rec* __restrict__ s, int64_t n, int64_t nv, const uint32_t* __restrict__ place,
                                                       uint32_t* __restrict__ begin, uint32_t* __restrict__ out, int64_t capacity,
                                                       uint8_t* __restrict__ boundary)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint64_t key = s[j].key;
    const int64_t v = record_vertex(key, kShift);
    if (v >= nv) return;
    const bool has_prev = j > 0, has_next = j + 1 < n;
    const uint64_t prev = has_prev ? s[j - 1].key : 0ull, next = has_next ? s[j + 1].key : 0ull;
    const bool entry = kShift == 0 || entry_head(key, has_prev, prev, nv, kShift);
    const uint32_t at = kShift == 0 ? (uint32_t)j : place[j];
    if (entry && (int64_t)at < capacity) out[at] = kShift == 0 ? s[j].index : (uint32_t)key;   // (always within)
    if (vertex_first(key, has_prev, prev, nv, kShift)) begin[v] = at;
    if (kShift == 32 && boundary && run_of_one(key, has_prev, prev, has_next, next)) {
        const int64_t w = (int64_t)(uint32_t)key;
        boundary[v] = 1;
        if (w < nv) boundary[w] = 1;   // (always: an index of the mesh; every writer stores the same byte)
    }
}

template <int kShift>
__global__ __launch_bounds__(kBlock) void k_ta_degree(const Rec* __restrict__ s, int64_t n, int64_t nv, const uint32_t* __restrict__ place,
                                                      const uint32_t* __restrict__ begin, uint32_t* __restrict__ degree)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint64_t key = s[j].key;
    const int64_t v = record_vertex(key, kShift);
    if (v >= nv) return;
    const bool has_next = j + 1 < n;
    if (vertex_last(key, has_next, has_next ? s[j + 1].key : 0ull, nv, kShift))
        degree[v] = (kShift == 0 ? (uint32_t)(j + 1) : place[j + 1]) - begin[v];
}

// ---- the gathers ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_tv_step(const float* __restrict__ pos, const uint32_t* __restrict__ nbr_start,
                                                    const uint32_t* __restrict__ nbr, const uint8_t* __restrict__ pin, int64_t nv, float s,
                                                    float* __restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    float r[3];
    smooth_vertex(pos, nbr, nbr_start[v], nbr_start[v + 1], pin && pin[v] != 0, s, v, r);
    __builtin_memcpy(out + 3 * v, r, sizeof r);
}

__global__ __launch_bounds__(kBlock) void k_tv_normals(const float* __restrict__ pos, const int32_t* __restrict__ idx,
                                                       const uint32_t* __restrict__ inc_start, const uint32_t* __restrict__ inc, int64_t nv, int flip,
                                                       float* __restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    float r[3];
    vertex_normal(pos, idx, inc, inc_start[v], inc_start[v + 1], flip != 0, r);
    out[3 * v] = r[0]; out[3 * v + 1] = r[1]; out[3 * v + 2] = r[2];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// One of the two structures, once per handle: synchronises (the number of entries sizes the list).
int csr_prepare(sdfk_trimesh* t, bool corners, const char* who)
{
    if (corners ? t->inc_start != nullptr : t->nbr_start != nullptr) return SDFK_OK;
    const int64_t nv = t->nv, nt = t->nt, n = (corners ? 3 : 6) * nt;
    Staged st;
    Rec* ra = st.scratch<Rec>((size_t)n);
    Rec* rb = st.scratch<Rec>((size_t)n);
    Rec* sorted = nullptr;
    uint32_t* head = corners ? nullptr : st.scratch<uint32_t>((size_t)n + 1);   // (neighbours) the head flags, scanned: the place of every entry
    uint32_t* begin = st.scratch<uint32_t>((size_t)nv);                        // the first place of every vertex that has a record
    uint32_t* start = st.kept<uint32_t>((size_t)nv + 1);                       // for the handle: degrees, scanned
    uint8_t* boundary = corners ? nullptr : st.kept<uint8_t>((size_t)nv);      // for the handle (neighbours)
    uint32_t entries = 0, total = 0;
    int64_t capacity = 3 * nt;
    st.run([&] {
        ProfScope ps(corners ? "k_ta_corner_keys" : "k_ta_nbr_keys");
        if (corners) hipLaunchKernelGGL(k_ta_corner_keys, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->idx, nt, nv, ra);
        else hipLaunchKernelGGL(k_ta_nbr_keys, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->idx, nt, nv, ra);
    });
    st.run([&] { return radix_sort(ra, rb, n, corners ? corner_digit_mask(nv) : nbr_digit_mask(nv), &sorted, who); });
    if (!corners) {
        ProfScope ps("k_ta_heads");
        st.run([&] { hipLaunchKernelGGL(k_ta_heads, dim3(grid1(n)), dim3(kBlock), 0, g.stream, sorted, n, nv, head); });
        st.run([&] { return sdfk_scan::scan(head, n, who); });
        st.read(&entries, head + n, sizeof entries);
        capacity = std::max<int64_t>((int64_t)entries, 1);
    }
    uint32_t* list = st.kept<uint32_t>((size_t)capacity);   // for the handle
    st.run([&] { return hipMemsetAsync(start, 0, (size_t)(nv + 1) * sizeof(uint32_t), g.stream); });
    if (boundary) st.run([&] { return hipMemsetAsync(boundary, 0, (size_t)nv, g.stream); });
    {
        ProfScope ps("k_ta_entries");
        st.run([&] {
            if (corners) {
                hipLaunchKernelGGL(k_ta_entries<0>, dim3(grid1(n)), dim3(kBlock), 0, g.stream, sorted, n, nv, nullptr, begin, list, capacity, nullptr);
                hipLaunchKernelGGL(k_ta_degree<0>, dim3(grid1(n)), dim3(kBlock), 0, g.stream, sorted, n, nv, nullptr, begin, start);
            } else {
                hipLaunchKernelGGL(k_ta_entries<32>, dim3(grid1(n)), dim3(kBlock), 0, g.stream, sorted, n, nv, head, begin, list, capacity, boundary);
                hipLaunchKernelGGL(k_ta_degree<32>, dim3(grid1(n)), dim3(kBlock), 0, g.stream, sorted, n, nv, head, begin, start);
            }
        });
        st.run([&] { return sdfk_scan::scan(start, nv, who); });
        st.read(&total, start + nv, sizeof total);
    }
    st.run([&] {   // (no input reaches this)
        return (int64_t)total > capacity ? fail(SDFK_ERR_INVALID, "%s: the degrees do not add up to the entries", who) : (int)SDFK_OK;
    });
    if (int r = st.finish(who, false)) return r;   // (the read above has waited; start, list and boundary are the handle's from here)
    if (corners) {
        t->inc_start = start; t->inc = list; t->inc_entries = (int64_t)total;
    } else {
        t->nbr_start = start; t->nbr = list; t->boundary = boundary; t->nbr_entries = (int64_t)total;
    }
    return SDFK_OK;
}

int smooth_check(const sdfk_trimesh* t, int32_t iterations, float lambda, float mu, int32_t flags, const void* out, const char* who)
{
    if (int r = trimesh_check(t, who, 6)) return r;
    if (!out) return fail(SDFK_ERR_INVALID, "%s: null output", who);
    if (iterations < 0 || iterations > 65536) return fail(SDFK_ERR_INVALID, "%s: iterations must be in [0, 65536]", who);
    if (!std::isfinite(lambda) || !std::isfinite(mu)) return fail(SDFK_ERR_INVALID, "%s: lambda and mu must be finite", who);
    if (flags & ~SDFK_TRIMESH_SMOOTH_PIN_BOUNDARY) return fail(SDFK_ERR_INVALID, "%s: unknown flag bits", who);
    return SDFK_OK;
}

// out: device memory, nv x 3.  Queues every step; waits for nothing once the handle has its adjacency.
int smooth(sdfk_trimesh* t, int32_t iterations, float lambda, float mu, int32_t flags, float* out, const char* who)
{
    const int64_t nv = t->nv, steps = smooth_steps(iterations, mu);
    hipError_t e = hipSuccess;
    if (steps == 0) {
        e = hipMemcpyAsync(out, t->vertices, (size_t)nv * 3 * sizeof(float), hipMemcpyDeviceToDevice, g.stream);
        if (e != hipSuccess) return fail(SDFK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
        return SDFK_OK;
    }
    if (int r = csr_prepare(t, false, who)) return r;
    Staged st;
    float* tmp = steps >= 2 ? st.scratch<float>((size_t)nv * 3) : nullptr;
    const uint8_t* pin = (flags & SDFK_TRIMESH_SMOOTH_PIN_BOUNDARY) ? t->boundary : nullptr;
    st.run([&] {
        ProfScope ps("k_tv_step");
        const float* src = t->vertices;
        for (int64_t i = 0; i < steps; i++) {
            float* dst = ((steps - 1 - i) & 1) ? tmp : out;   // (the last step writes the output)
            hipLaunchKernelGGL(k_tv_step, dim3(grid1(nv)), dim3(kBlock), 0, g.stream, src, t->nbr_start, t->nbr, pin, nv,
                               smooth_factor(i, lambda, mu), dst);
            src = dst;
        }
    });
    return st.finish(who, false);   // (the temporary goes back to the stream-ordered pool under the queued steps)
}

int normals_check(const sdfk_trimesh* t, int32_t flags, const void* out, const char* who)
{
    if (int r = trimesh_check(t, who, 6)) return r;
    if (!out) return fail(SDFK_ERR_INVALID, "%s: null output", who);
    if (flags & ~SDFK_TRIMESH_NORMALS_FLIP) return fail(SDFK_ERR_INVALID, "%s: unknown flag bits", who);
    return SDFK_OK;
}

// positions: device memory (null: the handle's own); out: device memory
int normals(sdfk_trimesh* t, const float* positions, int32_t flags, float* out, const char* who)
{
    if (int r = csr_prepare(t, true, who)) return r;
    {
        ProfScope ps("k_tv_normals");
        hipLaunchKernelGGL(k_tv_normals, dim3(grid1(t->nv)), dim3(kBlock), 0, g.stream, positions ? positions : t->vertices, t->idx, t->inc_start,
                           t->inc, t->nv, flags & SDFK_TRIMESH_NORMALS_FLIP, out);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SDFK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return SDFK_OK;
}

int adjacency_out(sdfk_trimesh* t, void* nbr_start, void* nbr, void* boundary, int64_t* n_entries, bool device, const char* who)
{
    if (int r = trimesh_check(t, who, 6)) return r;
    if (int r = csr_prepare(t, false, who)) return r;
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    Staged st;   // (no device copies: the adjacency is the handle's, and goes straight into the caller's arrays)
    if (nbr_start) st.run([&] { return hipMemcpyAsync(nbr_start, t->nbr_start, (size_t)(t->nv + 1) * sizeof(uint32_t), kind, g.stream); });
    if (nbr && t->nbr_entries) st.run([&] { return hipMemcpyAsync(nbr, t->nbr, (size_t)t->nbr_entries * sizeof(uint32_t), kind, g.stream); });
    if (boundary) st.run([&] { return hipMemcpyAsync(boundary, t->boundary, (size_t)t->nv, kind, g.stream); });
    if (int r = st.finish(who, !device)) return r;   // (the device form waits for nothing)
    if (n_entries) *n_entries = t->nbr_entries;
    return SDFK_OK;
}

}  // namespace

int trimesh_corners(sdfk_trimesh* t, const char* who) { return csr_prepare(t, true, who); }   // (trimesh_handle.h)

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_trimesh_adjacency_device(sdfk_trimesh* t, void* nbr_start_dev, void* nbr_dev, void* boundary_dev, int64_t* n_entries)
{
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return adjacency_out(t, nbr_start_dev, nbr_dev, boundary_dev, n_entries, true, "sdfk_trimesh_adjacency");
}

extern "C" int sdfk_trimesh_adjacency(sdfk_trimesh* t, uint32_t* nbr_start, uint32_t* nbr, uint8_t* boundary, int64_t* n_entries)
{
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return adjacency_out(t, nbr_start, nbr, boundary, n_entries, false, "sdfk_trimesh_adjacency");
}

extern "C" int sdfk_trimesh_smooth_device(sdfk_trimesh* t, int32_t iterations, float lambda, float mu, int32_t flags, void* vertices3_out_dev)
{
    static const char* who = "sdfk_trimesh_smooth";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = smooth_check(t, iterations, lambda, mu, flags, vertices3_out_dev, who)) return r;
    return smooth(t, iterations, lambda, mu, flags, (float*)vertices3_out_dev, who);
}

extern "C" int sdfk_trimesh_smooth(sdfk_trimesh* t, int32_t iterations, float lambda, float mu, int32_t flags, float* vertices3_out)
{
    static const char* who = "sdfk_trimesh_smooth";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = smooth_check(t, iterations, lambda, mu, flags, vertices3_out, who)) return r;
    Staged st;
    float* od = st.out(vertices3_out, (size_t)t->nv * 3);
    st.run([&] { return smooth(t, iterations, lambda, mu, flags, od, who); });
    return st.finish(who);
}

extern "C" int sdfk_trimesh_vertex_normals_device(sdfk_trimesh* t, const void* positions3_dev, int32_t flags, void* normals3_out_dev)
{
    static const char* who = "sdfk_trimesh_vertex_normals";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = normals_check(t, flags, normals3_out_dev, who)) return r;
    return normals(t, (const float*)positions3_dev, flags, (float*)normals3_out_dev, who);
}

extern "C" int sdfk_trimesh_vertex_normals(sdfk_trimesh* t, const float* positions3, int32_t flags, float* normals3_out)
{
    static const char* who = "sdfk_trimesh_vertex_normals";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = normals_check(t, flags, normals3_out, who)) return r;
    Staged st;
    float* od = st.out(normals3_out, (size_t)t->nv * 3);
    const float* pd = st.in(positions3, (size_t)t->nv * 3);   // (null: the handle's own vertices)
    st.run([&] { return normals(t, pd, flags, od, who); });
    return st.finish(who);
}
