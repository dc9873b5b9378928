// lib_orient.hip -- a consistent orientation of point-cloud normals (sdfk_points_orient_normals*): a parallel, deterministic
// region growing over the k-nearest graph, confident edges first.  Contract: include/sdfkit_hip.h, "Point clouds: a consistent
// orientation"; the decisions (validity, dot, the seed's order and sign, one point's choice from its row, the level rule):
// points_orient.h, checked on the host; the walk, the tiers and the bounded lists: points_walk.h / points_knn.h, shared with every
// query of the KdTree; the scratch of a call and the reads of the control block: a Staged (device_stage.h).
//
//   k_or_rows<CAP>   one lane per static point: its k nearest exactly as k_pts_knn<CAP> finds them (the same tiers), written once
//                    for the call as SLOT-MAJOR rows (slot * n + point; -1 from the count on): in a round lane i reads slot s of
//                    its own row, so neighbouring lanes read neighbouring words.  Also the point's state: stamp 0, sign byte 0
//                    (invalid normal) or +1, and the count of valid normals.
//   k_or_seed_find   the unoriented valid point of greatest (z, lowest index) as ONE integer key (points_orient.h seed_key):
//                    a shuffle maximum per wave, then an integer atomicMax -- no float atomics, the result is order-free.
//   k_or_seed_apply  one lane: the seed's sign and stamp, level 0.
//   k_or_round       one lane per point; a lane whose point is oriented or invalid leaves at once.  The others scan their row
//                    for sources (0 < stamp < this launch's number), take the one of greatest |dot| and, if its weight reaches
//                    the level's threshold, write their sign byte and stamp.
// State: one int32 stamp per point (0: unoriented, else the number of the launch that oriented it) and a sign byte -- the Jacobi
// rule without a second buffer: a stamp written concurrently in launch q reads as 0 or q, and both mean "not yet".
// Schedule: every launch (seed or round) takes the next number q.  The control block keeps, in rings of three indexed by q % 3,
// the level launch q ran at and how many points it oriented: launch q reads slot q - 1 (written by the launch before it, so the
// stream order is the only hand-off), writes slot q and clears slot q + 1.  The level of launch q follows on the device
// (points_orient.h next_level); once it passes the last level the growth of the seed is over and every later round of the batch
// leaves after those two loads.  The host queues rounds kBatch at a time and reads the control block once per batch; the same
// read tells it whether the seed's growth ended and whether unoriented valid points remain for another seed.
// Rounds that left early are not counted: stats[0] counts seeds and live rounds only, whatever the batch length.
#include "lib_internal.h"
#include "device_wave.h"
#include "points_knn.h"
#include "points_orient.h"
#include "points_set.h"
#include "points_walk.h"

namespace {

using namespace sdfk_walk;
using namespace sdfk_orient;

constexpr int kBatch = 32;   // rounds queued between two reads of the control block (tests/test_gpu_orient.py BATCH repeats it: keep them equal)

struct Ctl {
    unsigned long long seed_key;             // k_or_seed_find's maximum; 0: no candidate (cleared by k_or_seed_apply)
    unsigned long long rounds, seeds;        // live rounds (seed rounds included), seeds
    unsigned long long valid;                // valid normals
    unsigned long long flipped, unreached;   // k_or_finish
    unsigned long long per_level[kLevels];   // points oriented at each level
    int level[3];                            // ring by launch number: the level launch q ran at (kLevels: growth over)
    unsigned count[3];                       // ring: the points launch q oriented
};

template <int CAP>
__global__ __launch_bounds__(block_of<CAP>()) void k_or_rows(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                              const float* __restrict__ xyz, int64_t n, int k, float d2_bound,
                                                              const float* __restrict__ normals, int32_t* __restrict__ rows,
                                                              int32_t* __restrict__ stamp, signed char* __restrict__ sgn, Ctl* ctl)
{
    __shared__ uint64_t s_keys[lds_keys<CAP>()];
    const int64_t t = (int64_t)blockIdx.x * block_of<CAP>() + threadIdx.x;
    const Query q = load_query(xyz, t, n);
    Neighbours<CAP> nb;
    (void)nb.collect(sorted, starts, G, q, k, d2_bound, s_keys);
    bool ok = false;
    if (t < n) {
        int slot = 0;
        nb.each([&](uint64_t key) {
            rows[(int64_t)slot * n + t] = key_index(key);
            slot++;
            return true;
        });
        for (; slot < k; slot++) rows[(int64_t)slot * n + t] = -1;
        float nrm[3];
        load3(normals, t, nrm);
        ok = valid(nrm);
        stamp[t] = 0;
        sgn[t] = ok ? 1 : 0;
    }
    const unsigned c = wave_count(ok);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ctl->valid, (unsigned long long)c);
}

__global__ __launch_bounds__(kBlock) void k_or_seed_find(const float* __restrict__ xyz, int64_t n, const int32_t* __restrict__ stamp,
                                                         const signed char* __restrict__ sgn, Ctl* ctl)
{
    unsigned long long best = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        if (sgn[i] != 0 && stamp[i] == 0) {
            const unsigned long long key = seed_key(xyz[3 * i + 2], (int32_t)i);
            best = key > best ? key : best;
        }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_down(best, o);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0 && best) atomicMax(&ctl->seed_key, best);
}

__global__ __launch_bounds__(64) void k_or_seed_apply(int q, const float* __restrict__ normals, int32_t* __restrict__ stamp,
                                                      signed char* __restrict__ sgn, Ctl* ctl)
{
    if (threadIdx.x != 0) return;
    const unsigned long long key = ctl->seed_key;
    ctl->seed_key = 0;
    ctl->count[(q + 1) % 3] = 0;
    if (!key) {   // no unoriented valid point: nothing grows
        ctl->level[q % 3] = kLevels;
        ctl->count[q % 3] = 0;
        return;
    }
    const int32_t i = seed_index(key);
    float nrm[3];
    load3(normals, i, nrm);
    sgn[i] = (signed char)seed_sign(nrm);
    stamp[i] = q;
    ctl->level[q % 3] = 0;
    ctl->count[q % 3] = 1;   // (the round after a seed stays at level 0)
    ctl->rounds += 1;
    ctl->seeds += 1;
}

__global__ __launch_bounds__(kBlock) void k_or_round(const int32_t* __restrict__ rows, int64_t n, int k, int q, const float* __restrict__ normals,
                                                     int32_t* stamp, signed char* sgn, Ctl* ctl)
{
    const int prev = (q + 2) % 3, cur = q % 3;
    const int level = next_level(__atomic_load_n(&ctl->level[prev], __ATOMIC_RELAXED), __atomic_load_n(&ctl->count[prev], __ATOMIC_RELAXED));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->level[cur] = level;
        ctl->count[(q + 1) % 3] = 0;
        if (level < kLevels) ctl->rounds += 1;
    }
    if (level >= kLevels) return;   // the growth of this seed ended before this launch
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool did = false;
    if (i < n && sgn[i] != 0 && stamp[i] == 0) {
        float ni[3];
        load3(normals, i, ni);
        Choice c;
        for (int s = 0; s < k; s++) {
            const int32_t j = rows[(int64_t)s * n + i];
            if (j < 0) break;
            const int32_t st = __atomic_load_n(&stamp[j], __ATOMIC_RELAXED);
            if (st > 0 && st < q) {   // (oriented before this launch: its sign byte is final; tested here to spare the loads of the others)
                float nj[3];
                load3(normals, j, nj);
                if (is_source(st, q, nj)) c.offer(ni, nj, (int)sgn[j]);
            }
        }
        if (c.accepted(level)) {
            sgn[i] = (signed char)c.sign();
            __atomic_store_n(&stamp[i], q, __ATOMIC_RELAXED);
            did = true;
        }
    }
    const unsigned cnt = wave_count(did);
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicAdd(&ctl->count[cur], cnt);
        atomicAdd(&ctl->per_level[level], (unsigned long long)cnt);
    }
}

__global__ __launch_bounds__(kBlock) void k_or_finish(int64_t n, float* __restrict__ normals, const int32_t* __restrict__ stamp,
                                                      const signed char* __restrict__ sgn, Ctl* ctl)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool flip = false, unreached = false;
    if (i < n) {
        const signed char s = sgn[i];
        flip = s < 0;
        unreached = s != 0 && stamp[i] == 0;
        if (flip)
            for (int a = 0; a < 3; a++) normals[3 * i + a] = flipped(normals[3 * i + a]);
    }
    const unsigned cf = wave_count(flip), cu = wave_count(unreached);
    if ((threadIdx.x & 63) == 0) {
        if (cf) atomicAdd(&ctl->flipped, (unsigned long long)cf);
        if (cu) atomicAdd(&ctl->unreached, (unsigned long long)cu);
    }
}

int orient(const sdfk_points* s, int k, float max_distance, int64_t max_seeds, float* normals, int64_t stats[9])
{
    static const char* who = "sdfk_points_orient_normals";
    const int64_t n = s->n;
    Staged st;
    int32_t* rows = st.scratch<int32_t>((size_t)n * (size_t)k);
    int32_t* stamp = st.scratch<int32_t>((size_t)n);
    signed char* sgn = st.scratch<signed char>((size_t)n);
    Ctl* ctl = st.scratch<Ctl>(1);
    Ctl host{};
    st.run([&] { return hipMemsetAsync(ctl, 0, sizeof(Ctl), g.stream); });
    st.run([&] {
        ProfScope ps("k_or_rows");
        const float d2b = radius_d2_bound(max_distance);
        launch_tier(k, n, [&](auto cap, dim3 grid, dim3 block) {
            hipLaunchKernelGGL(k_or_rows<decltype(cap)::value>, grid, block, 0, g.stream, s->sorted, s->starts, s->G, s->xyz, n, k, d2b, normals, rows, stamp, sgn, ctl);
        });
    });
    const unsigned blocks = grid_of(n, kBlock);
    int64_t q = 0;   // launches numbered so far
    const auto bounded = [&] { return q > (int64_t(1) << 30) ? fail(SDFK_ERR_INVALID, "%s: 2^30 rounds without an end", who) : (int)SDFK_OK; };
    while (st.ok()) {
        st.run([&] {
            ProfScope ps("k_or_seed");
            q++;
            hipLaunchKernelGGL(k_or_seed_find, dim3((unsigned)grid_for((size_t)n, kBlock, 2048)), dim3(kBlock), 0, g.stream, s->xyz, n, stamp, sgn, ctl);
            hipLaunchKernelGGL(k_or_seed_apply, dim3(1), dim3(64), 0, g.stream, (int)q, normals, stamp, sgn, ctl);
        });
        while (st.ok()) {   // this seed's growth, a batch at a time
            st.run([&] {
                ProfScope ps("k_or_round");
                for (int b = 0; b < kBatch; b++) {
                    q++;
                    hipLaunchKernelGGL(k_or_round, dim3(blocks), dim3(kBlock), 0, g.stream, rows, n, k, (int)q, normals, stamp, sgn, ctl);
                }
            });
            st.read(&host, ctl, sizeof host);
            if (!st.ok() || host.level[q % 3] >= kLevels) break;   // the last queued round found the growth over
            st.run(bounded);
        }
        if (!st.ok()) break;
        unsigned long long oriented = host.seeds;
        for (int l = 0; l < kLevels; l++) oriented += host.per_level[l];
        if (oriented >= host.valid || (int64_t)host.seeds >= max_seeds) break;
        st.run(bounded);
    }
    {
        ProfScope ps("k_or_finish");
        st.run([&] { hipLaunchKernelGGL(k_or_finish, dim3(blocks), dim3(kBlock), 0, g.stream, n, normals, stamp, sgn, ctl); });
        if (stats) st.read(&host, ctl, sizeof host);
    }
    if (int r = st.finish(who, false)) return r;   // (no wait of its own: with stats the read above was one)
    if (stats) {
        stats[0] = (int64_t)host.rounds;
        stats[1] = (int64_t)host.seeds;
        stats[2] = (int64_t)host.flipped;
        stats[3] = (int64_t)host.unreached;
        stats[4] = n - (int64_t)host.valid;
        for (int l = 0; l < kLevels; l++) stats[5 + l] = (int64_t)host.per_level[l];
    }
    return SDFK_OK;
}

int check_orient(const sdfk_points* s, int32_t k, float max_distance, int32_t max_seeds, const void* normals, int64_t stats[9])
{
    static const char* who = "sdfk_points_orient_normals";
    if (int r = require_init()) return r;
    if (!s) return fail(SDFK_ERR_INVALID, "%s: null point set", who);
    if (k < kMinK || k > kMaxK) return fail(SDFK_ERR_INVALID, "%s: k = %d is outside [%d, %d]", who, (int)k, kMinK, kMaxK);
    if (!radius_is_valid(max_distance)) return fail(SDFK_ERR_INVALID, "%s: max_distance is negative or NaN", who);
    if (max_seeds < 1) return fail(SDFK_ERR_INVALID, "%s: max_seeds = %d, at least 1 is needed", who, (int)max_seeds);
    if (!normals) return fail(SDFK_ERR_INVALID, "%s: null normals", who);
    if (stats)
        for (int i = 0; i < 9; i++) stats[i] = 0;
    return SDFK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_points_orient_normals_device(const sdfk_points* s, int32_t k, float max_distance, int32_t max_seeds, void* normals3_dev,
                                                 int64_t stats[9])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_orient(s, k, max_distance, max_seeds, normals3_dev, stats)) return r;
    return orient(s, k, max_distance, max_seeds, (float*)normals3_dev, stats);
}

extern "C" int sdfk_points_orient_normals(const sdfk_points* s, int32_t k, float max_distance, int32_t max_seeds, float* normals3, int64_t stats[9])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_orient(s, k, max_distance, max_seeds, normals3, stats)) return r;
    Staged st;
    float* nd = st.inout(normals3, (size_t)s->n * 3);
    st.run([&] { return orient(s, k, max_distance, max_seeds, nd, stats); });
    return st.finish("sdfk_points_orient_normals");
}
