// points_walk.h -- the owner of the KdTree's shell walk: the one walk over the grid of sorted cell lists that lib_points.hip builds,
// with its conservative lower bound, run by every query kernel (lib_points.hip: nearest point, ICP; lib_points_knn.hip: k nearest,
// within a radius; lib_pointcloud.hip: normals, volumes; lib_orient.hip: neighbour rows; lib_points_filter.hip: mean neighbour
// distances) through a visitor.  Also what the k-nearest kernels share: the visitor that keeps the k least keys, the LDS storage of
// the heap tiers and the launch of a kernel's tier for k; the one grid computation of the family (grid_of); and walk_launch, the
// launch of a walk kernel under its span with the candidate counter of a profiled call.  The arithmetic of keys, lists and the
// k-nearest stopping rule is points_knn.h's.  hipcc only.
#pragma once
#include "lib_internal.h"
#include "device_wave.h"
#include "points_knn.h"
#include "points_set.h"

#include <algorithm>
#include <cfloat>
#include <type_traits>

namespace sdfk_walk {

using namespace sdfk_points_grid;
using namespace sdfk_knn;

constexpr int kBlock = 256;     // the register tier and the radius kernels
constexpr int kLdsBlock = 64;   // the LDS tiers: one wave per block

// the conservative lower bound of d2 over the unvisited cells: beyond the shell along one axis (the nearer of its two gaps) and
// outside the box along the other two
__device__ __forceinline__ float lb_sq(const float gap[3][2], const float base2[3])
{
    float best = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float rest = base2[(a + 1) % 3] + base2[(a + 2) % 3];
        const float gm = fminf(gap[a][0], gap[a][1]);
        best = fminf(best, gm * gm + rest);
    }
    return best;
}

// The walk of a finite query: one lane, cells in growing Chebyshev shells around the query's cell (clamped to the grid).
// V::take(d2, s) per candidate s = (x, y, z, bits(index)); V::done(lb2) after each shell, lb2 the lower bound of d2 over every
// unvisited cell.  Returns the number of candidates.
template <class V>
__device__ __forceinline__ unsigned long long shell_walk(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, const Grid& G,
                                                         float qx, float qy, float qz, V& v)
{
    unsigned long long ncand = 0;
    const float q[3] = {qx, qy, qz};
    int c[3];
    (void)key_of(G, qx, qy, qz, &c[0], &c[1], &c[2]);
    const float slack = G.slack + fmaxf(fabsf(qx), fmaxf(fabsf(qy), fabsf(qz))) * 0x1p-20f;
    float base2[3];
    int rmax = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float out = fmaxf(fmaxf(G.lo[a] - q[a], q[a] - G.hi[a]) - slack, 0.0f);
        base2[a] = out * out;
        rmax = max(rmax, max(c[a], G.dim[a] - 1 - c[a]));
    }
    const int gx = G.dim[0], gy = G.dim[1];
    for (int r = 0; r <= rmax; r++) {
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, G.dim[2] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, gy - 1);
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, gx - 1);
        for (int z = z0; z <= z1; z++) {
            const bool zf = z == c[2] - r || z == c[2] + r;
            for (int y = y0; y <= y1; y++) {
                const bool full = zf || y == c[1] - r || y == c[1] + r;
                const uint32_t row = ((uint32_t)z * (uint32_t)gy + (uint32_t)y) * (uint32_t)gx;
                // a full row of the shell is one contiguous range of the sorted points; otherwise its two end cells
                for (int part = 0; part < (full ? 1 : 2); part++) {
                    int xa, xb;
                    if (full) { xa = x0; xb = x1; }
                    else {
                        xa = xb = part == 0 ? c[0] - r : c[0] + r;
                        if (xa < 0 || xa >= gx) continue;
                    }
                    const uint32_t j0 = starts[row + (uint32_t)xa], j1 = starts[row + (uint32_t)xb + 1];
                    ncand += j1 - j0;
                    for (uint32_t j = j0; j < j1; j++) {
                        const float4 s = sorted[j];
                        v.take(dist2(qx, qy, qz, s.x, s.y, s.z), s);
                    }
                }
            }
        }
        // every unvisited cell lies beyond shell r along some axis: the least distance it can have, made conservative
        float gap[3][2];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            gap[a][0] = c[a] - r - 1 >= 0 ? fmaxf(q[a] - (G.lo[a] + (float)(c[a] - r) * G.h) - slack, 0.0f) : INFINITY;
            gap[a][1] = c[a] + r + 1 < G.dim[a] ? fmaxf((G.lo[a] + (float)(c[a] + r + 1) * G.h) - q[a] - slack, 0.0f) : INFINITY;
        }
        if (v.done(lb_sq(gap, base2))) break;
    }
    return ncand;
}

struct Query {
    float x, y, z;
    bool finite;
};
__device__ __forceinline__ Query load_query(const float* __restrict__ queries, int64_t t, int64_t nq)
{
    Query q{NAN, NAN, NAN, false};
    if (t < nq) { q.x = queries[3 * t]; q.y = queries[3 * t + 1]; q.z = queries[3 * t + 2]; }
    q.finite = isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
    return q;
}

__device__ __forceinline__ void load3(const float* __restrict__ a, int64_t i, float out[3])
{
    out[0] = a[3 * i]; out[1] = a[3 * i + 1]; out[2] = a[3 * i + 2];
}

// ---- k nearest ---------------------------------------------------------------------------------------------------------------
struct LdsSlots {   // slot-major keys of one lane
    uint64_t* base;   // &s_keys[lane]
    __device__ __forceinline__ uint64_t get(int i) const { return base[i * kLdsBlock]; }
    __device__ __forceinline__ void set(int i, uint64_t key) { base[i * kLdsBlock] = key; }
};

template <class L>
struct KnnVisitor {
    L list;
    uint64_t bound_key;   // (radius bound, index all ones): the greatest key within the radius
    float d2_bound;
    __device__ __forceinline__ void take(float d2, const float4& s)
    {
        const uint64_t key = pack_key(d2, __float_as_int(s.w));
        if (key <= bound_key && key < list.worst()) list.insert(key);
    }
    __device__ __forceinline__ bool done(float lb2) const { return walk_done(lb2, list.worst(), d2_bound); }
};

// The k nearest of one query as a finished list (ascending; at(i) = kKeyInf from the count on), for the kernels that go on
// working on the neighbours.  CAP = 8: the sorted list in registers (at(i) wants a constant i); otherwise the heap in `lds`, the
// block's CAP * kLdsBlock keys.  Returns the number of candidates.
template <int CAP>
struct Neighbours {
    using List = typename std::conditional<CAP == 8, SortedList<8>, HeapList<LdsSlots>>::type;
    KnnVisitor<List> v;
    int m;   // neighbours found
    __device__ __forceinline__ unsigned long long collect(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, const Grid& G,
                                                          const Query& q, int k, float d2_bound, uint64_t* lds)
    {
        if constexpr (CAP != 8) v.list.s.base = &lds[threadIdx.x];
        v.list.init(k);
        v.bound_key = pack_key(d2_bound, -1);
        v.d2_bound = d2_bound;
        unsigned long long ncand = 0;
        if (q.finite) ncand = shell_walk(sorted, starts, G, q.x, q.y, q.z, v);
        v.list.finish();
        m = v.list.count();
        return ncand;
    }
    // f(key) for the neighbours in order, while f returns true
    template <class F>
    __device__ __forceinline__ void each(F&& f) const
    {
        if constexpr (CAP == 8) {
            bool go = true;
#pragma unroll
            for (int i = 0; i < 8; i++)
                if (go && i < m) go = f(v.list.at(i));
        } else {
            for (int i = 0; i < m; i++)
                if (!f(v.list.at(i))) break;
        }
    }
    // f(i, key) for the slots i < k of an output row: the neighbours in order, then kKeyInf (constant i in the register tier)
    template <class F>
    __device__ __forceinline__ void each_slot(int k, F&& f) const
    {
        if constexpr (CAP == 8) {
#pragma unroll
            for (int i = 0; i < 8; i++)
                if (i < k) f(i, v.list.at(i));
        } else {
            for (int i = 0; i < k; i++) f(i, v.list.at(i));
        }
    }
    __device__ __forceinline__ uint64_t last() const   // the m-th key (m >= 1)
    {
        if constexpr (CAP == 8) {
            uint64_t key = v.list.at(0);
#pragma unroll
            for (int i = 1; i < 8; i++) key = i < m ? v.list.at(i) : key;
            return key;
        } else
            return v.list.at(m - 1);
    }
};

inline unsigned grid_of(int64_t n, int block) { return (unsigned)std::max<int64_t>(1, (n + block - 1) / block); }

// a tiered kernel's block, and the keys its block holds in LDS
template <int CAP>
constexpr int block_of() { return CAP == 8 ? kBlock : kLdsBlock; }
template <int CAP>
constexpr int lds_keys() { return CAP == 8 ? 1 : CAP * kLdsBlock; }   // (the register tier keeps no keys in LDS)

// The launch of a tiered kernel for k over n lanes: launch(cap, grid, block) with cap an std::integral_constant<int, CAP>.
template <class F>
inline void launch_tier(int k, int64_t n, F&& launch)
{
    auto go = [&](auto cap) {
        constexpr int B = block_of<decltype(cap)::value>();
        launch(cap, dim3(grid_of(n, B)), dim3(B));
    };
    switch (tier_of(k)) {
    case 8: go(std::integral_constant<int, 8>{}); break;
    case 16: go(std::integral_constant<int, 16>{}); break;
    case 32: go(std::integral_constant<int, 32>{}); break;
    default: go(std::integral_constant<int, 64>{}); break;
    }
}

// The launch of a walk kernel (or of the tiers of one): launch(counter) queues it under the span `name`, counter being the device
// word its lanes add their candidates to -- null unless profiling is on (and `counted`), when the call zeroes it before, and reads
// it into sdfk_points_stats[3..4] with the nq queries after (which synchronises).  launch returns nothing, or the SDFK_ERR_* of
// what it queued besides.  The counter is a ProfCount of a Staged of this call (device_stage.h), which reports SDFK_OK or the
// failure as "<who>: <error string>": the launch's HIP error before the counter's, then what launch returned.  A call that failed
// -- a HIP error or an SDFK_ERR_* from launch alike -- waits for the stream, as every Staged does, and leaves the stats as they were.
template <class F>
inline int walk_launch(const sdfk_points* s, int64_t nq, const char* name, const char* who, F&& launch, bool counted = true)
{
    Staged st;
    ProfCount<1> pc;
    pc.begin(st, counted && g.prof_on);
    int r = SDFK_OK;
    st.run([&] {   // (a step that returns nothing: the launch's HIP error is taken first, what launch returned comes after the counter)
        ProfScope ps(name);
        if constexpr (std::is_void<decltype(launch(pc.dev))>::value) launch(pc.dev);
        else r = launch(pc.dev);
    });
    unsigned long long c[1];
    const bool read = pc.end(st, c);
    st.run([&] { return r; });
    if (int rf = st.finish(who, false)) return rf;
    if (read) {
        const_cast<sdfk_points*>(s)->last_candidates = (int64_t)c[0];
        const_cast<sdfk_points*>(s)->last_queries = nq;
    }
    return SDFK_OK;
}

}  // namespace sdfk_walk
