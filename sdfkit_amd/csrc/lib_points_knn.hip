// lib_points_knn.hip -- KdTree's k-nearest and radius queries (sdfk_points_knn*, sdfk_points_radius_*) over the grid of sorted
// cell lists that lib_points.hip builds.  Contract: include/sdfkit_hip.h, "k nearest / within a radius"; the arithmetic (packed
// (d2, index) keys, bounded lists, radius predicate, stopping rule): points_knn.h, checked on the host.
//
// One lane per query on the family's one shell walk (points_walk.h), the walk k_pts_search runs too, launched as every walk kernel
// is (walk_launch); a kernel is the visitor it hands the walk -- what a candidate meets and when the walk stops:
//   k_pts_knn<CAP>       the k least keys within the radius bound; stops when the lower bound of every unvisited cell exceeds the
//                        k-th key's d2 (+inf until k are held) or the radius bound.  CAP = 8: a sorted list in registers; CAP = 16 /
//                        32 / 64: a max-heap in LDS, slot-major (slot * 64 + lane: conflict-free across the wave), ordered in place
//                        at the end.  Blocks of one wave: LDS per block = CAP * 512 B, so 20 / 10 / 5 waves per CU (160 KiB).
//   k_pts_radius_count   the number of points within the bound; an exclusive 64-bit scan (device_scan.h) makes the offsets.
//   k_pts_radius_fill    the same walk writes (index, bits(d2)) into the query's segment of the caller's arrays, a per-lane
//                        in-place heap sort on the packed keys orders it, then d2 becomes the distance.  Without a distance
//                        array the sort recomputes d2 from the stored index (bit-identical: the same formula on the same floats).
#include "lib_internal.h"
#include "device_scan.h"
#include "points_knn.h"
#include "points_set.h"
#include "points_walk.h"

#include <cfloat>

namespace {

using namespace sdfk_walk;   // the shell walk, the k-nearest visitor, the LDS slots, the profiled launch

// ---- k nearest ---------------------------------------------------------------------------------------------------------------
struct KnnOut {
    int32_t* index;     // n x k; any may be null
    float* distance;    // n x k
    int32_t* found;     // n
    unsigned long long* candidates;
};

template <int CAP>
__global__ __launch_bounds__(block_of<CAP>()) void k_pts_knn(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                              const float* __restrict__ queries, int64_t nq, int k, float d2_bound, KnnOut O)
{
    __shared__ uint64_t s_keys[lds_keys<CAP>()];
    const int64_t t = (int64_t)blockIdx.x * block_of<CAP>() + threadIdx.x;
    const Query q = load_query(queries, t, nq);
    Neighbours<CAP> nb;
    const unsigned long long ncand = nb.collect(sorted, starts, G, q, k, d2_bound, s_keys);
    if (t < nq) {
        int32_t* const irow = O.index ? O.index + t * k : nullptr;
        float* const drow = O.distance ? O.distance + t * k : nullptr;
        nb.each_slot(k, [&](int i, uint64_t key) {
            const bool real = key < kKeyInf;
            if (irow) irow[i] = real ? key_index(key) : -1;
            if (drow) drow[i] = real ? sqrt_rn(key_d2(key)) : FLT_MAX;
        });
        if (O.found) O.found[t] = nb.m;
    }
    wave_add(O.candidates, ncand);
}

// ---- within a radius ---------------------------------------------------------------------------------------------------------
struct CountVisitor {
    float d2_bound;
    unsigned long long n;
    __device__ __forceinline__ void take(float d2, const float4&) { n += within(d2, d2_bound) ? 1u : 0u; }
    __device__ __forceinline__ bool done(float lb2) const { return walk_done(lb2, kKeyInf, d2_bound); }
};

// counts[t] = neighbours of query t (the scan turns them into offsets in place)
__global__ __launch_bounds__(kBlock) void k_pts_radius_count(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                             const float* __restrict__ queries, int64_t nq, float d2_bound,
                                                             unsigned long long* __restrict__ counts, unsigned long long* candidates)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const Query q = load_query(queries, t, nq);
    CountVisitor v{d2_bound, 0};
    unsigned long long ncand = 0;
    if (q.finite) ncand = shell_walk(sorted, starts, G, q.x, q.y, q.z, v);
    if (t < nq) counts[t] = v.n;
    wave_add(candidates, ncand);
}

// a query's segment as heap storage.  WITH_D2: the d2 bits live in the distance array until the end.
template <bool WITH_D2>
struct Segment {
    int32_t* index;
    uint32_t* d2bits;      // WITH_D2
    const float* xyz;      // !WITH_D2: the static points in insertion order
    float qx, qy, qz;
    __device__ __forceinline__ uint64_t get(int i) const
    {
        const int32_t id = index[i];
        if constexpr (WITH_D2) return (uint64_t)d2bits[i] << 32 | (uint32_t)id;
        else return pack_key(dist2(qx, qy, qz, xyz[3 * (int64_t)id], xyz[3 * (int64_t)id + 1], xyz[3 * (int64_t)id + 2]), id);
    }
    __device__ __forceinline__ void set(int i, uint64_t key)
    {
        index[i] = key_index(key);
        if constexpr (WITH_D2) d2bits[i] = (uint32_t)(key >> 32);
    }
};

template <bool WITH_D2>
struct FillVisitor {
    Segment<WITH_D2> seg;
    float d2_bound;
    int64_t n, cap;   // written so far, the segment's length (a segment is never overrun, whatever the offsets say)
    __device__ __forceinline__ void take(float d2, const float4& s)
    {
        if (within(d2, d2_bound) && n < cap) {
            seg.index[n] = __float_as_int(s.w);
            if constexpr (WITH_D2) seg.d2bits[n] = f32_bits(d2);
            n++;
        }
    }
    __device__ __forceinline__ bool done(float lb2) const { return walk_done(lb2, kKeyInf, d2_bound); }
};

template <bool WITH_D2>
__global__ __launch_bounds__(kBlock) void k_pts_radius_fill(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                            const float* __restrict__ xyz, const float* __restrict__ queries, int64_t nq,
                                                            float d2_bound, const int64_t* __restrict__ offsets, int32_t* __restrict__ index,
                                                            float* __restrict__ distance, unsigned long long* candidates)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const Query q = load_query(queries, t, nq);
    unsigned long long ncand = 0;
    if (q.finite) {
        const int64_t o0 = offsets[t], o1 = offsets[t + 1];
        FillVisitor<WITH_D2> v;
        v.seg = Segment<WITH_D2>{index + o0, WITH_D2 ? (uint32_t*)distance + o0 : nullptr, xyz, q.x, q.y, q.z};
        v.d2_bound = d2_bound;
        v.n = 0;
        v.cap = o1 > o0 ? o1 - o0 : 0;
        ncand = shell_walk(sorted, starts, G, q.x, q.y, q.z, v);
        const int m = (int)v.n;   // (< 2^31: the static points)
        heap_make(v.seg, m);
        heap_sort(v.seg, m);
        if constexpr (WITH_D2)
            for (int i = 0; i < m; i++) v.seg.d2bits[i] = f32_bits(sqrt_rn(bits_f32(v.seg.d2bits[i])));   // d2 -> distance, in place
    }
    wave_add(candidates, ncand);
}

// ---- launches ----------------------------------------------------------------------------------------------------------------

int knn_launch(const sdfk_points* s, const float* q, int64_t nq, int k, float d2_bound, KnnOut O)
{
    return walk_launch(s, nq, "k_pts_knn", "sdfk_points_knn", [&](unsigned long long* counter) {
        O.candidates = counter;
        launch_tier(k, nq, [&](auto cap, dim3 grid, dim3 block) {
            hipLaunchKernelGGL(k_pts_knn<decltype(cap)::value>, grid, block, 0, g.stream, s->sorted, s->starts, s->G, q, nq, k, d2_bound, O);
        });
    });
}

// offsets_dev[0 .. nq]: the counts, scanned in place
int count_launch(const sdfk_points* s, const float* q, int64_t nq, float d2_bound, int64_t* offsets_dev)
{
    static const char* who = "sdfk_points_radius_count";
    unsigned long long* off = reinterpret_cast<unsigned long long*>(offsets_dev);
    return walk_launch(s, nq, "k_pts_radius_count", who, [&](unsigned long long* counter) {
        hipLaunchKernelGGL(k_pts_radius_count, dim3(grid_of(nq, kBlock)), dim3(kBlock), 0, g.stream, s->sorted, s->starts, s->G, q, nq, d2_bound, off,
                           counter);
        return sdfk_scan::scan(off, nq, who);
    });
}

int fill_launch(const sdfk_points* s, const float* q, int64_t nq, float d2_bound, const int64_t* offsets_dev, int32_t* index, float* distance)
{
    return walk_launch(s, nq, "k_pts_radius_fill", "sdfk_points_radius_fill", [&](unsigned long long* counter) {
        if (distance)
            hipLaunchKernelGGL(k_pts_radius_fill<true>, dim3(grid_of(nq, kBlock)), dim3(kBlock), 0, g.stream, s->sorted, s->starts, s->G, s->xyz, q, nq,
                               d2_bound, offsets_dev, index, distance, counter);
        else
            hipLaunchKernelGGL(k_pts_radius_fill<false>, dim3(grid_of(nq, kBlock)), dim3(kBlock), 0, g.stream, s->sorted, s->starts, s->G, s->xyz, q, nq,
                               d2_bound, offsets_dev, index, distance, counter);
    });
}

int check_queries(const sdfk_points* s, const void* queries, int64_t n, const char* who)
{
    if (int r = require_init()) return r;
    if (!s || n < 0 || (n > 0 && !queries)) return fail(SDFK_ERR_INVALID, "%s: null / negative argument", who);
    if (n >= (int64_t(1) << 32)) return fail(SDFK_ERR_INVALID, "%s: 2^32 queries or more", who);
    return SDFK_OK;
}

int check_knn(const sdfk_points* s, const void* queries, int64_t n, int32_t k, float max_distance)
{
    if (int r = check_queries(s, queries, n, "sdfk_points_knn")) return r;
    if (k < 1 || k > kMaxK) return fail(SDFK_ERR_INVALID, "sdfk_points_knn: k = %d is outside [1, %d] (larger neighbourhoods: sdfk_points_radius_*)", (int)k, kMaxK);
    if (!radius_is_valid(max_distance)) return fail(SDFK_ERR_INVALID, "sdfk_points_knn: max_distance is negative or NaN");
    return SDFK_OK;
}

int check_radius(const sdfk_points* s, const void* queries, int64_t n, float radius, const void* offsets, const char* who)
{
    if (int r = check_queries(s, queries, n, who)) return r;
    if (!offsets) return fail(SDFK_ERR_INVALID, "%s: null offsets", who);
    if (!radius_is_valid(radius)) return fail(SDFK_ERR_INVALID, "%s: the radius is negative or NaN", who);
    return SDFK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_points_knn_device(const sdfk_points* s, const void* queries3_dev, int64_t n, int32_t k, float max_distance, void* index_dev,
                                      void* distance_dev, void* found_dev)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_knn(s, queries3_dev, n, k, max_distance)) return r;
    if (n == 0) return SDFK_OK;
    return knn_launch(s, (const float*)queries3_dev, n, k, radius_d2_bound(max_distance), KnnOut{(int32_t*)index_dev, (float*)distance_dev, (int32_t*)found_dev, nullptr});
}

extern "C" int sdfk_points_knn(const sdfk_points* s, const float* queries3, int64_t n, int32_t k, float max_distance, int32_t* index, float* distance,
                               int32_t* found)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_knn(s, queries3, n, k, max_distance)) return r;
    if (n == 0) return SDFK_OK;
    const size_t nk = (size_t)n * (size_t)k;
    Staged st;
    const float* qd = st.in(queries3, (size_t)n * 3);
    const KnnOut O{st.out(index, nk), st.out(distance, nk), st.out(found, (size_t)n), nullptr};
    st.run([&] { return knn_launch(s, qd, n, k, radius_d2_bound(max_distance), O); });
    return st.finish("sdfk_points_knn");
}

extern "C" int sdfk_points_radius_count_device(const sdfk_points* s, const void* queries3_dev, int64_t n, float radius, void* offsets_dev)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_radius(s, queries3_dev, n, radius, offsets_dev, "sdfk_points_radius_count")) return r;
    if (n == 0) {
        if (hipMemsetAsync(offsets_dev, 0, sizeof(int64_t), g.stream) != hipSuccess) return fail(SDFK_ERR_HIP, "sdfk_points_radius_count: memset");
        return SDFK_OK;
    }
    return count_launch(s, (const float*)queries3_dev, n, radius_d2_bound(radius), (int64_t*)offsets_dev);
}

extern "C" int sdfk_points_radius_count(const sdfk_points* s, const float* queries3, int64_t n, float radius, int64_t* offsets)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_radius(s, queries3, n, radius, offsets, "sdfk_points_radius_count")) return r;
    if (n == 0) {
        offsets[0] = 0;
        return SDFK_OK;
    }
    Staged st;
    const float* qd = st.in(queries3, (size_t)n * 3);
    int64_t* od = st.out(offsets, (size_t)n + 1);
    st.run([&] { return count_launch(s, qd, n, radius_d2_bound(radius), od); });
    return st.finish("sdfk_points_radius_count");
}

extern "C" int sdfk_points_radius_fill_device(const sdfk_points* s, const void* queries3_dev, int64_t n, float radius, const void* offsets_dev,
                                              void* index_dev, void* distance_dev)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_radius(s, queries3_dev, n, radius, offsets_dev, "sdfk_points_radius_fill")) return r;
    if (n == 0) return SDFK_OK;
    if (!index_dev) return fail(SDFK_ERR_INVALID, "sdfk_points_radius_fill: null index");
    return fill_launch(s, (const float*)queries3_dev, n, radius_d2_bound(radius), (const int64_t*)offsets_dev, (int32_t*)index_dev, (float*)distance_dev);
}

extern "C" int sdfk_points_radius_fill(const sdfk_points* s, const float* queries3, int64_t n, float radius, const int64_t* offsets, int32_t* index,
                                       float* distance)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_radius(s, queries3, n, radius, offsets, "sdfk_points_radius_fill")) return r;
    if (n == 0) return SDFK_OK;
    // the host form sizes its device arrays by offsets[n]: offsets that do not start at 0 and ascend to it would leave them
    const int64_t total = offsets[n];
    if (offsets[0] != 0) return fail(SDFK_ERR_INVALID, "sdfk_points_radius_fill: offsets[0] is not 0");
    for (int64_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return fail(SDFK_ERR_INVALID, "sdfk_points_radius_fill: offsets do not ascend (at query %lld)", (long long)i);
    if (total == 0) return SDFK_OK;
    if (!index) return fail(SDFK_ERR_INVALID, "sdfk_points_radius_fill: null index");
    Staged st;
    const float* qd = st.in(queries3, (size_t)n * 3);
    const int64_t* od = st.in(offsets, (size_t)n + 1);
    int32_t* id = st.out(index, (size_t)total);
    float* dd = st.out(distance, (size_t)total);
    st.run([&] { return fill_launch(s, qd, n, radius_d2_bound(radius), od, id, dd); });
    return st.finish("sdfk_points_radius_fill");
}
