// device_sort.h -- the stable LSD radix sort of 16-byte (key, index) records that the voxel filter (lib_points_filter.hip), the
// edge census and the adjacency of a triangle mesh (lib_trimesh_topology.hip, lib_trimesh_smooth.hip) and its welding
// (lib_trimesh_weld.hip) share: 8-bit digits, only the passes the caller's mask names.  Per
// pass the digit counts of every tile of kSortTile records (LDS counters; integer adds, order-free), digit-major, one exclusive
// scan over all of them (device_scan.h), then the scatter; how the scatter keeps equal digits in order is told at
// lib_points_filter.hip's head.  Each unit that includes this gets its own copy of the two kernels.  hipcc only.
#pragma once
#include "lib_internal.h"
#include "device_scan.h"

namespace {

constexpr int kSortBlock = 256;
constexpr int kSortRounds = 8;                                // rounds of 64 records per wave
constexpr int kSortTile = kSortBlock * kSortRounds;           // 2048 records (tests/test_gpu_points_filter.py TILE repeats it)
constexpr int kSortWave = 64 * kSortRounds;                   // a wave's contiguous part of the tile

struct alignas(16) Rec {
    unsigned long long key;
    uint32_t index, pad;
};

// hist[digit * ntiles + tile] = records of the tile with that digit
__global__ __launch_bounds__(kSortBlock) void k_rs_hist(const Rec* __restrict__ in, int64_t n, int shift, uint32_t ntiles, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t s_cnt[256];
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kSortTile;
    for (int j = 0; j < kSortRounds; j++) {
        const int64_t i = base + j * kSortBlock + threadIdx.x;
        if (i < n) atomicAdd(&s_cnt[(unsigned)(in[i].key >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = s_cnt[threadIdx.x];
}

// offs: the scanned histogram
__global__ __launch_bounds__(kSortBlock) void k_rs_scatter(const Rec* __restrict__ in, Rec* __restrict__ out, int64_t n, int shift, uint32_t ntiles,
                                                           const uint32_t* __restrict__ offs)
{
    __shared__ uint32_t s_wave[4][256];   // [wave][digit]: the wave's running count, then its first destination
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = 0; j < 4; j++) s_wave[j][threadIdx.x] = 0;
    __syncthreads();
    const int64_t wbase = (int64_t)blockIdx.x * kSortTile + (int64_t)w * kSortWave + lane;
    const unsigned long long lower = (1ull << lane) - 1ull;
    Rec r[kSortRounds];
    uint32_t rank[kSortRounds];
#pragma unroll
    for (int j = 0; j < kSortRounds; j++) {
        const int64_t i = wbase + j * 64;
        const bool valid = i < n;
        r[j] = valid ? in[i] : Rec{0ull, 0u, 0u};
        const unsigned digit = (unsigned)(r[j].key >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long has = __ballot(valid && bit);
            peers &= bit ? has : ~has;
        }
        const uint32_t before = valid ? s_wave[w][digit] : 0u;
        __builtin_amdgcn_wave_barrier();   // (every peer has read the count before the first of them raises it)
        const uint32_t below = (uint32_t)__popcll(peers & lower);
        if (valid && below == 0) s_wave[w][digit] = before + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        rank[j] = before + below;
    }
    __syncthreads();
    {
        const unsigned d = threadIdx.x;   // one digit per lane: the waves' counts -> the first destination of each wave's run
        uint32_t run = offs[(size_t)d * ntiles + blockIdx.x];
        for (int j = 0; j < 4; j++) {
            const uint32_t c = s_wave[j][d];
            s_wave[j][d] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSortRounds; j++) {
        const int64_t i = wbase + j * 64;
        if (i < n) {
            const unsigned digit = (unsigned)(r[j].key >> shift) & 255u;
            const uint32_t dest = s_wave[w][digit] + rank[j];
            if (dest < n) out[dest] = r[j];   // (always: the histogram counted these same records)
        }
    }
}

// Sorts the n records of a by key, stably, through the passes of `mask`; -> the buffer that holds the result (a or b).
int radix_sort(Rec* a, Rec* b, int64_t n, unsigned mask, Rec** sorted, const char* who)
{
    *sorted = a;
    if (!mask) return SDFK_OK;
    const uint32_t ntiles = (uint32_t)((n + kSortTile - 1) / kSortTile);
    const int64_t nh = (int64_t)ntiles * 256;
    uint32_t* hist = nullptr;
    if (int r = dev_alloc((void**)&hist, (size_t)(nh + 1) * sizeof(uint32_t))) return r;
    int r = SDFK_OK;
    for (int d = 0; d < 8 && !r; d++) {
        if (!(mask >> d & 1u)) continue;
        ProfScope ps("k_rs_pass");
        hipLaunchKernelGGL(k_rs_hist, dim3(ntiles), dim3(kSortBlock), 0, g.stream, a, n, 8 * d, ntiles, hist);
        r = sdfk_scan::scan(hist, nh, who);
        if (r) break;
        hipLaunchKernelGGL(k_rs_scatter, dim3(ntiles), dim3(kSortBlock), 0, g.stream, a, b, n, 8 * d, ntiles, hist);
        std::swap(a, b);
    }
    dev_free(hist);
    *sorted = a;
    return r;
}

}  // namespace
