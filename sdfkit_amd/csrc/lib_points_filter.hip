// lib_points_filter.hip -- the KdTree's two filters: sdfk_points_voxel_downsample* (one centroid per occupied voxel of a
// world-anchored lattice; sdfk_points_voxel_downsample_colors*: and the members' mean colour) and sdfk_points_outliers* (the
// statistical outlier rule over the k-nearest rows).  Contract: include/sdfkit_hip.h, "Point clouds: filters" and "Point clouds:
// colours"; the arithmetic (voxel, range check, packed key, chunked centroid sum, row mean, threshold, keep rule): points_filter.h,
// (the mean colour): points_color.h, both checked on the host; the walk, the tiers and the bounded lists: points_walk.h /
// points_knn.h, shared with every query of the KdTree; the integer scan of the sort and of both compactions: device_scan.h.
//
// Downsample:
//   k_vf_keys      one lane per point: (packed key, insertion index) as one 16-byte record.
//   k_rs_hist      (device_sort.h, shared with lib_trimesh_topology.hip) a stable LSD radix sort of the records, 8-bit digits, only the digits the three ranges can set (the host knows
//   k_rs_scatter   them): per pass the digit counts of every tile of kSortTile records (LDS counters; integer adds, order-free),
//                  digit-major, one exclusive scan over all of them, then the scatter.  A tile is 4 waves x 8 rounds of 64
//                  consecutive records; wave w owns the w-th quarter of the tile.  In a round the lanes of equal digit find each
//                  other with 8 ballots; a lane's rank is the wave's running count of its digit (LDS, one row per wave, touched by
//                  that wave only, in program order) plus the peers in lower lanes -- so equal digits keep their order within the
//                  wave, the wave rows are prefixed in wave order, and the tiles in tile order by the scan: the sort is stable, and
//                  from the identity it leaves every voxel's members in ascending index.  One 16-byte store per record.
//   k_vf_heads     head flag of every sorted position (its key differs from the one before), and the same flag at the member's
//                  insertion index: a voxel's head is its lowest member.  Two scans: segment numbers in key order, and output
//                  numbers in the order of the lowest members.  The host reads m here.
//   k_vf_starts    the start of every segment.
//   k_vf_chunks    one lane per chunk of 32 members: its three sums (a lane per sorted position; chunk starts go on).
//   k_vf_finish    one lane per sorted position: group of its point; at a head the chunk sums in order, the centroid, the count.
//   k_vc_chunks    with colours only: the same segments and chunk slots, the three sums of the members' colours;
//   k_vc_finish    at a head the chunk sums in order and the mean colour.  The sort and the segments are the centroids'.
// Outliers:
//   k_of_mean<CAP> one lane per static point on the shell walk (the tiers of k_pts_knn): the row's mean distance in binary64.
//   k_of_sum / k_of_var / k_of_thr   the fixed-order reductions of device_reduce.h, as the ICP's: sum and count, squared
//                  deviations, then mu, sigma and the threshold.
//   k_of_flags     keep byte, flag and (float)mean; a scan; k_of_scatter writes the kept indices and points.
// Host side: the scratch and the host forms' device copies are held in a Staged (device_stage.h).
#include "lib_internal.h"
#include "device_reduce.h"
#include "device_scan.h"
#include "device_sort.h"
#include "points_color.h"
#include "points_filter.h"
#include "points_knn.h"
#include "points_set.h"
#include "points_walk.h"

namespace {

using namespace sdfk_walk;
using namespace sdfk_filter;

// ---- the radix sort: device_sort.h ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_vf_keys(const float* __restrict__ xyz, int64_t n, Lattice L, Rec* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = Rec{voxel_key(L, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]), (uint32_t)i, 0u};
}

// ---- voxel downsample --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_head(const Rec* __restrict__ s, int64_t j) { return j == 0 || s[j].key != s[j - 1].key; }

__global__ __launch_bounds__(kBlock) void k_vf_heads(const Rec* __restrict__ s, int64_t n, uint32_t* __restrict__ seg, uint32_t* __restrict__ first)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t h = is_head(s, j) ? 1u : 0u;
    seg[j] = h;
    first[s[j].index] = h;   // (every index once: the array is written whole)
}

// seg: scanned.  start[0 .. m]: the sorted position each segment begins at, start[m] = n.
__global__ __launch_bounds__(kBlock) void k_vf_starts(const Rec* __restrict__ s, int64_t n, const uint32_t* __restrict__ seg, uint32_t m,
                                                      uint32_t* __restrict__ start)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    if (is_head(s, j) && seg[j] < m) start[seg[j]] = (uint32_t)j;
    if (j == 0) start[m] = (uint32_t)n;
}

// the slot of chunk q of segment `sid`, which starts at sorted position hs: ascending over all chunks, below n / 32 + m + 1
__device__ __forceinline__ int64_t chunk_slot(uint32_t hs, uint32_t sid, uint32_t q) { return (int64_t)(hs >> 5) + sid + q; }

__global__ __launch_bounds__(kBlock) void k_vf_chunks(const Rec* __restrict__ s, int64_t n, const uint32_t* __restrict__ seg,
                                                      const uint32_t* __restrict__ start, uint32_t m, const float* __restrict__ xyz,
                                                      double* __restrict__ csum, int64_t slots)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t sid = seg[j] + (is_head(s, j) ? 1u : 0u) - 1u;
    if (sid >= m) return;
    const uint32_t hs = start[sid], end = start[sid + 1];
    const uint32_t rel = (uint32_t)j - hs;
    if (rel % kChunk != 0 || end > n) return;
    const int count = (int)min((uint32_t)kChunk, end - (uint32_t)j);
    Sum3 sum;
    for (int t = 0; t < count; t++) {
        const int64_t id = s[j + t].index;
        sum.add_point(xyz[3 * id], xyz[3 * id + 1], xyz[3 * id + 2]);
    }
    const int64_t slot = chunk_slot(hs, sid, rel / kChunk);
    if (slot < slots)
        for (int a = 0; a < 3; a++) csum[3 * slot + a] = sum.v[a];
}

// first: scanned (first[i] of a voxel's lowest member i = the voxel's output number)
__global__ __launch_bounds__(kBlock) void k_vf_finish(const Rec* __restrict__ s, int64_t n, const uint32_t* __restrict__ seg,
                                                      const uint32_t* __restrict__ start, uint32_t m, const uint32_t* __restrict__ first,
                                                      const double* __restrict__ csum, int64_t slots, float* __restrict__ points_out,
                                                      int32_t* __restrict__ counts, int32_t* __restrict__ group)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const bool head = is_head(s, j);
    const uint32_t sid = seg[j] + (head ? 1u : 0u) - 1u;
    if (sid >= m) return;
    const uint32_t hs = start[sid], end = start[sid + 1];
    if (hs >= n || end > n) return;
    const uint32_t o = first[s[hs].index];
    if (o >= m) return;
    if (group) group[s[j].index] = (int32_t)o;
    if (!head) return;
    const int64_t count = (int64_t)end - (int64_t)hs;
    if (counts) counts[o] = (int32_t)count;
    if (points_out) {
        const int64_t chunks = chunks_of(count), base = chunk_slot(hs, sid, 0);
        Sum3 total;
        for (int64_t q = 0; q < chunks && base + q < slots; q++) total.add_sum(&csum[3 * (base + q)]);
        for (int a = 0; a < 3; a++) points_out[3 * (int64_t)o + a] = centroid_of(total.v[a], count);
    }
}

// the colours of the same segments: one lane per chunk of 32 members, as k_vf_chunks
__global__ __launch_bounds__(kBlock) void k_vc_chunks(const Rec* __restrict__ s, int64_t n, const uint32_t* __restrict__ seg,
                                                      const uint32_t* __restrict__ start, uint32_t m, const float* __restrict__ colors3,
                                                      double* __restrict__ csum, int64_t slots)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t sid = seg[j] + (is_head(s, j) ? 1u : 0u) - 1u;
    if (sid >= m) return;
    const uint32_t hs = start[sid], end = start[sid + 1];
    const uint32_t rel = (uint32_t)j - hs;
    if (rel % kChunk != 0 || end > n) return;
    const int count = (int)min((uint32_t)kChunk, end - (uint32_t)j);
    const Sum3 sum = sdfk_color::chunk_sum(colors3, count, [&](int t) { return (int64_t)s[j + t].index; });
    const int64_t slot = chunk_slot(hs, sid, rel / kChunk);
    if (slot < slots)
        for (int a = 0; a < 3; a++) csum[3 * slot + a] = sum.v[a];
}

// one lane per sorted position; a head writes its voxel's mean colour
__global__ __launch_bounds__(kBlock) void k_vc_finish(const Rec* __restrict__ s, int64_t n, const uint32_t* __restrict__ seg,
                                                      const uint32_t* __restrict__ start, uint32_t m, const uint32_t* __restrict__ first,
                                                      const double* __restrict__ csum, int64_t slots, float* __restrict__ colors_out)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n || !is_head(s, j)) return;
    const uint32_t sid = seg[j];
    if (sid >= m) return;
    const uint32_t hs = start[sid], end = start[sid + 1];
    if (hs >= n || end > n || end <= hs) return;
    const uint32_t o = first[s[hs].index];
    if (o >= m) return;
    const int64_t count = (int64_t)end - (int64_t)hs, base = chunk_slot(hs, sid, 0);
    if (base + chunks_of(count) > slots) return;   // (never: the slots were sized for every chunk)
    float rgb[3];
    sdfk_color::group_mean(count, [&](int64_t q) { return &csum[3 * (base + q)]; }, rgb);
    for (int a = 0; a < 3; a++) colors_out[3 * (int64_t)o + a] = rgb[a];
}

struct DownArgs {
    Lattice L;
    unsigned mask;   // the sort's passes
};

int check_downsample(const sdfk_points* s, float size, const float origin[3], DownArgs* A)
{
    static const char* who = "sdfk_points_voxel_downsample";
    if (int r = require_init()) return r;
    if (!s) return fail(SDFK_ERR_INVALID, "%s: null point set", who);
    if (!size_is_valid(size)) return fail(SDFK_ERR_INVALID, "%s: the voxel size is not a finite positive number", who);
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const float* o = origin ? origin : zero;
    if (!origin_is_valid(o)) return fail(SDFK_ERR_INVALID, "%s: the origin is not finite", who);
    int bits[3];
    A->L.size = size;
    for (int a = 0; a < 3; a++) {
        A->L.origin[a] = o[a];
        // the voxel of a coordinate is monotone in it and the box's corners are coordinates of points: the extreme voxels
        const double kmin = voxel_of(s->G.lo[a], o[a], size), kmax = voxel_of(s->G.hi[a], o[a], size);
        if (!span_is_valid(kmin, kmax))
            return fail(SDFK_ERR_INVALID, "%s: the points span 2^21 voxels or more along axis %d (a larger voxel size is needed)", who, a);
        A->L.kmin[a] = kmin;
        bits[a] = span_bits(kmin, kmax);
    }
    A->mask = digit_mask(bits);
    return SDFK_OK;
}

// everything on the device; *m_out is read on the way (the call is synchronous).  colors3 / colors_out: both or neither.
int downsample(const sdfk_points* s, const DownArgs& A, float* points_out, int32_t* counts, int32_t* group, int64_t* m_out,
               const float* colors3 = nullptr, float* colors_out = nullptr)
{
    const char* who = colors3 ? "sdfk_points_voxel_downsample_colors" : "sdfk_points_voxel_downsample";
    const int64_t n = s->n;
    Staged st;
    Rec* ra = st.scratch<Rec>((size_t)n);
    Rec* rb = st.scratch<Rec>((size_t)n);
    Rec* sorted = nullptr;
    uint32_t* seg = st.scratch<uint32_t>((size_t)n + 1);
    uint32_t* first = st.scratch<uint32_t>((size_t)n + 1);
    uint32_t m = 0;
    st.run([&] {
        ProfScope ps("k_vf_keys");
        hipLaunchKernelGGL(k_vf_keys, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, s->xyz, n, A.L, ra);
    });
    st.run([&] { return radix_sort(ra, rb, n, A.mask, &sorted, who); });
    {
        ProfScope ps("k_vf_heads");
        st.run([&] { hipLaunchKernelGGL(k_vf_heads, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, sorted, n, seg, first); });
        st.run([&] { return sdfk_scan::scan(seg, n, who); });
        st.run([&] { return sdfk_scan::scan(first, n, who); });
    }
    st.read(&m, seg + n, sizeof m);
    const int64_t slots = n / kChunk + (int64_t)m + 2;
    uint32_t* start = st.scratch<uint32_t>((size_t)m + 1);
    double* csum = points_out ? st.scratch<double>((size_t)slots * 3) : nullptr;
    double* ccsum = colors_out ? st.scratch<double>((size_t)slots * 3) : nullptr;
    st.run([&] {
        ProfScope ps("k_vf_centroids");
        hipLaunchKernelGGL(k_vf_starts, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, sorted, n, seg, m, start);
        if (points_out)
            hipLaunchKernelGGL(k_vf_chunks, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, sorted, n, seg, start, m, s->xyz, csum, slots);
        hipLaunchKernelGGL(k_vf_finish, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, sorted, n, seg, start, m, first, csum, slots, points_out, counts, group);
        if (colors_out) {
            hipLaunchKernelGGL(k_vc_chunks, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, sorted, n, seg, start, m, colors3, ccsum, slots);
            hipLaunchKernelGGL(k_vc_finish, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, sorted, n, seg, start, m, first, ccsum, slots, colors_out);
        }
    });
    if (int r = st.finish(who)) return r;   // (synchronises: the call returns when finished)
    if (m_out) *m_out = (int64_t)m;
    return SDFK_OK;
}

// ---- statistical outliers ----------------------------------------------------------------------------------------------------
using namespace sdfk_reduce;   // the fixed-order reductions, both levels
static_assert(kBlock == kReduceBlock, "the reductions run in blocks of device_reduce.h's size");

struct OfState {
    double part[kReduceBlocks][3];   // per-block partials: sum of the means, their count, sum of squared deviations
    double mu, sigma, thr, c;
};

template <int CAP>
__global__ __launch_bounds__(block_of<CAP>()) void k_of_mean(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                              const float* __restrict__ xyz, int64_t n, int k, float d2_bound,
                                                              double* __restrict__ mean)
{
    __shared__ uint64_t s_keys[lds_keys<CAP>()];
    const int64_t t = (int64_t)blockIdx.x * block_of<CAP>() + threadIdx.x;
    const Query q = load_query(xyz, t, n);
    Neighbours<CAP> nb;
    (void)nb.collect(sorted, starts, G, q, k, d2_bound, s_keys);
    if (t >= n) return;
    double sum = 0.0;
    int slot = 0;
    nb.each([&](uint64_t key) {
        if (slot > 0) sum = sum + (double)sqrt_rn(key_d2(key));   // (the first entry, distance 0, is dropped)
        slot++;
        return true;
    });
    mean[t] = row_mean(sum, nb.m);
}

__global__ __launch_bounds__(kBlock) void k_of_sum(const double* __restrict__ mean, int64_t n, OfState* S)
{
    __shared__ double s[2][kBlock];
    double v[2];
    grid_sum(n, v, s, [&](int64_t i, double* acc) {
        const double m = mean[i];
        if (!is_isolated(m)) { acc[0] += m; acc[1] += 1.0; }
    });
    if (threadIdx.x == 0) { S->part[blockIdx.x][0] = v[0]; S->part[blockIdx.x][1] = v[1]; }
}

__global__ __launch_bounds__(kBlock) void k_of_var(const double* __restrict__ mean, int64_t n, OfState* S)
{
    __shared__ double s[2][kBlock];
    double t[2];
    sum_partials(S->part, 0, t, s);   // (every block alike)
    const double mu = threshold_of(t[0], 0.0, t[1], 0.0f).mu;
    __syncthreads();   // (s is reused)
    double v[1];
    grid_sum(n, v, s, [&](int64_t i, double* acc) {
        const double m = mean[i];
        if (!is_isolated(m)) {
            const double d = m - mu;
            acc[0] += d * d;
        }
    });
    if (threadIdx.x == 0) S->part[blockIdx.x][2] = v[0];
}

__global__ __launch_bounds__(kBlock) void k_of_thr(OfState* S, float std_ratio)
{
    __shared__ double s[3][kBlock];
    double t[3];
    sum_partials(S->part, 0, t, s);
    if (threadIdx.x != 0) return;
    const Threshold T = threshold_of(t[0], t[2], t[1], std_ratio);
    S->mu = T.mu; S->sigma = T.sigma; S->thr = T.thr; S->c = t[1];
}

__global__ __launch_bounds__(kBlock) void k_of_flags(const double* __restrict__ mean, int64_t n, const OfState* __restrict__ S,
                                                     float* __restrict__ mean_distance, uint8_t* __restrict__ keep, uint32_t* __restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double m = mean[i];
    const bool kp = is_kept(m, S->thr);
    if (mean_distance) mean_distance[i] = (float)m;
    if (keep) keep[i] = kp ? 1 : 0;
    flag[i] = kp ? 1u : 0u;
}

// flag: scanned
__global__ __launch_bounds__(kBlock) void k_of_scatter(const double* __restrict__ mean, int64_t n, const OfState* __restrict__ S,
                                                       const uint32_t* __restrict__ flag, const float* __restrict__ xyz,
                                                       int32_t* __restrict__ index_out, float* __restrict__ points_out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !is_kept(mean[i], S->thr)) return;
    const int64_t o = flag[i];
    if (o >= n) return;
    if (index_out) index_out[o] = (int32_t)i;
    if (points_out)
        for (int a = 0; a < 3; a++) points_out[3 * o + a] = xyz[3 * i + a];
}

int64_t f64_bits(double x)
{
    int64_t u;
    memcpy(&u, &x, sizeof u);
    return u;
}

int check_outliers(const sdfk_points* s, int32_t k, float std_ratio, float max_distance)
{
    static const char* who = "sdfk_points_outliers";
    if (int r = require_init()) return r;
    if (!s) return fail(SDFK_ERR_INVALID, "%s: null point set", who);
    if (k < 2 || k > kMaxK) return fail(SDFK_ERR_INVALID, "%s: k = %d is outside [2, %d]", who, (int)k, kMaxK);
    if (!ratio_is_valid(std_ratio)) return fail(SDFK_ERR_INVALID, "%s: std_ratio must be finite and not negative", who);
    if (!radius_is_valid(max_distance)) return fail(SDFK_ERR_INVALID, "%s: max_distance is negative or NaN", who);
    return SDFK_OK;
}

int outliers(const sdfk_points* s, int k, float std_ratio, float max_distance, float* mean_distance, uint8_t* keep, int32_t* index_out,
             float* points_out, int64_t* n_kept, int64_t stats[6])
{
    static const char* who = "sdfk_points_outliers";
    const int64_t n = s->n;
    Staged st;
    double* mean = st.scratch<double>((size_t)n);
    uint32_t* flag = st.scratch<uint32_t>((size_t)n + 1);
    OfState* S = st.scratch<OfState>(1);
    st.run([&] {
        ProfScope ps("k_of_mean");
        const float d2b = radius_d2_bound(max_distance);
        launch_tier(k, n, [&](auto cap, dim3 grid, dim3 block) {
            hipLaunchKernelGGL(k_of_mean<decltype(cap)::value>, grid, block, 0, g.stream, s->sorted, s->starts, s->G, s->xyz, n, k, d2b, mean);
        });
    });
    st.run([&] {
        ProfScope ps("k_of_stats");
        launch_grid_sum(k_of_sum, g.stream, mean, n, S);
        launch_grid_sum(k_of_var, g.stream, mean, n, S);
        hipLaunchKernelGGL(k_of_thr, dim3(1), dim3(kBlock), 0, g.stream, S, std_ratio);
    });
    {
        ProfScope ps("k_of_compact");
        st.run([&] { hipLaunchKernelGGL(k_of_flags, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, mean, n, S, mean_distance, keep, flag); });
        st.run([&] { return sdfk_scan::scan(flag, n, who); });
        if (index_out || points_out)
            st.run([&] { hipLaunchKernelGGL(k_of_scatter, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, mean, n, S, flag, s->xyz, index_out, points_out); });
    }
    uint32_t kept = 0;
    double sv[4] = {0, 0, 0, 0};   // mu, sigma, thr, c
    st.run([&] { return hipMemcpyAsync(sv, &S->mu, sizeof sv, hipMemcpyDeviceToHost, g.stream); });
    st.run([&] { return hipMemcpyAsync(&kept, flag + n, sizeof kept, hipMemcpyDeviceToHost, g.stream); });
    if (int r = st.finish(who)) return r;   // (synchronises: the count and the statistics are read, and the call returns when finished)
    if (n_kept) *n_kept = (int64_t)kept;
    if (stats) {
        const int64_t c = (int64_t)sv[3];
        stats[0] = (int64_t)kept;
        stats[1] = c - (int64_t)kept;
        stats[2] = n - c;
        stats[3] = f64_bits(sv[0]);
        stats[4] = f64_bits(sv[1]);
        stats[5] = f64_bits(sv[2]);
    }
    return SDFK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_points_voxel_downsample_device(const sdfk_points* s, float voxel_size, const float origin[3], void* points_out_dev,
                                                   void* counts_dev, void* group_dev, int64_t* m)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    DownArgs A;
    if (int r = check_downsample(s, voxel_size, origin, &A)) return r;
    return downsample(s, A, (float*)points_out_dev, (int32_t*)counts_dev, (int32_t*)group_dev, m);
}

extern "C" int sdfk_points_voxel_downsample(const sdfk_points* s, float voxel_size, const float origin[3], float* points_out, int32_t* counts,
                                            int32_t* group, int64_t* m)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    DownArgs A;
    if (int r = check_downsample(s, voxel_size, origin, &A)) return r;
    const size_t n = (size_t)s->n;
    Staged st;
    float* points_d = points_out ? st.scratch<float>(n * 3) : nullptr;
    int32_t* counts_d = counts ? st.scratch<int32_t>(n) : nullptr;
    int32_t* group_d = st.out(group, n);
    int64_t found = 0;
    st.run([&] {
        if (int r = downsample(s, A, points_d, counts_d, group_d, &found)) return r;
        hipError_t e = copy_out(points_out, points_d, (size_t)found * 3);   // (the m voxels only: the rest of the caller's arrays stays)
        if (e == hipSuccess) e = copy_out(counts, counts_d, (size_t)found);
        return e == hipSuccess ? SDFK_OK : fail(SDFK_ERR_HIP, "sdfk_points_voxel_downsample: %s", hipGetErrorString(e));
    });
    const int r = st.finish("sdfk_points_voxel_downsample");
    if (!r && m) *m = found;
    return r;
}

extern "C" int sdfk_points_voxel_downsample_colors_device(const sdfk_points* s, float voxel_size, const float origin[3], const void* colors3_dev,
                                                          void* points_out_dev, void* counts_dev, void* group_dev, void* colors_out_dev, int64_t* m)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    DownArgs A;
    if (int r = check_downsample(s, voxel_size, origin, &A)) return r;
    if (!colors3_dev) return fail(SDFK_ERR_INVALID, "sdfk_points_voxel_downsample_colors: null colours");
    return downsample(s, A, (float*)points_out_dev, (int32_t*)counts_dev, (int32_t*)group_dev, m, (const float*)colors3_dev, (float*)colors_out_dev);
}

extern "C" int sdfk_points_voxel_downsample_colors(const sdfk_points* s, float voxel_size, const float origin[3], const float* colors3,
                                                   float* points_out, int32_t* counts, int32_t* group, float* colors_out, int64_t* m)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    DownArgs A;
    if (int r = check_downsample(s, voxel_size, origin, &A)) return r;
    if (!colors3) return fail(SDFK_ERR_INVALID, "sdfk_points_voxel_downsample_colors: null colours");
    const size_t n = (size_t)s->n;
    Staged st;
    const float* colors_in = st.in(colors3, n * 3);
    float* points_d = points_out ? st.scratch<float>(n * 3) : nullptr;
    int32_t* counts_d = counts ? st.scratch<int32_t>(n) : nullptr;
    float* colors_d = colors_out ? st.scratch<float>(n * 3) : nullptr;
    int32_t* group_d = st.out(group, n);
    int64_t found = 0;
    st.run([&] {
        if (int r = downsample(s, A, points_d, counts_d, group_d, &found, colors_in, colors_d)) return r;
        hipError_t e = copy_out(points_out, points_d, (size_t)found * 3);   // (the m voxels only: the rest of the caller's arrays stays)
        if (e == hipSuccess) e = copy_out(counts, counts_d, (size_t)found);
        if (e == hipSuccess) e = copy_out(colors_out, colors_d, (size_t)found * 3);
        return e == hipSuccess ? SDFK_OK : fail(SDFK_ERR_HIP, "sdfk_points_voxel_downsample_colors: %s", hipGetErrorString(e));
    });
    const int r = st.finish("sdfk_points_voxel_downsample_colors");
    if (!r && m) *m = found;
    return r;
}

extern "C" int sdfk_points_outliers_device(const sdfk_points* s, int32_t k, float std_ratio, float max_distance, void* mean_distance_dev,
                                           void* keep_dev, void* index_out_dev, void* points_out_dev, int64_t* n_kept, int64_t stats[6])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_outliers(s, k, std_ratio, max_distance)) return r;
    return outliers(s, k, std_ratio, max_distance, (float*)mean_distance_dev, (uint8_t*)keep_dev, (int32_t*)index_out_dev, (float*)points_out_dev,
                    n_kept, stats);
}

extern "C" int sdfk_points_outliers(const sdfk_points* s, int32_t k, float std_ratio, float max_distance, float* mean_distance, uint8_t* keep,
                                    int32_t* index_out, float* points_out, int64_t* n_kept, int64_t stats[6])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_outliers(s, k, std_ratio, max_distance)) return r;
    const size_t n = (size_t)s->n;
    Staged st;
    float* mean_d = st.out(mean_distance, n);
    uint8_t* keep_d = st.out(keep, n);
    int32_t* index_d = index_out ? st.scratch<int32_t>(n) : nullptr;
    float* points_d = points_out ? st.scratch<float>(n * 3) : nullptr;
    int64_t kept = 0, stv[6] = {0, 0, 0, 0, 0, 0};
    st.run([&] {
        if (int r = outliers(s, k, std_ratio, max_distance, mean_d, keep_d, index_d, points_d, &kept, stv)) return r;
        hipError_t e = copy_out(index_out, index_d, (size_t)kept);   // (the kept ones only)
        if (e == hipSuccess) e = copy_out(points_out, points_d, (size_t)kept * 3);
        return e == hipSuccess ? SDFK_OK : fail(SDFK_ERR_HIP, "sdfk_points_outliers: %s", hipGetErrorString(e));
    });
    const int r = st.finish("sdfk_points_outliers");
    if (!r) {
        if (n_kept) *n_kept = kept;
        if (stats)
            for (int i = 0; i < 6; i++) stats[i] = stv[i];
    }
    return r;
}
