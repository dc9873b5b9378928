// device_scan.h -- the exclusive prefix scan of the counting sorts and compactions (lib_points.hip, lib_points_filter.hip,
// lib_points_knn.hip, lib_trimesh.hip): counts[0..m) -> starts[0..m] in place, starts[m] = the total.  Blocks of kScanItems values
// (256 lanes x 8), the block totals scanned by one block, then the block offsets added.  Integer types only: the result does not
// depend on the order of anything.  scan() is the one call: it owns the scratch of the block totals.  hipcc only.
#pragma once
#include "lib_internal.h"

#include <algorithm>
#include <cstdint>

namespace sdfk_scan {

constexpr int kScanBlock = 256;
constexpr int kScanItems = kScanBlock * 8;

inline int64_t scan_blocks(int64_t m) { return std::max<int64_t>(1, (m + kScanItems - 1) / kScanItems); }

// Hillis-Steele over the block's 256 values
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* s_tmp, T* total)
{
    s_tmp[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < kScanBlock; o <<= 1) {
        const T a = (int)threadIdx.x >= o ? s_tmp[threadIdx.x - o] : T(0);
        __syncthreads();
        s_tmp[threadIdx.x] += a;
        __syncthreads();
    }
    const T incl = s_tmp[threadIdx.x];
    *total = s_tmp[kScanBlock - 1];
    __syncthreads();
    return incl - v;
}

template <typename T>
__global__ __launch_bounds__(kScanBlock) void k_scan_blocks(T* __restrict__ buf, int64_t m, T* __restrict__ block_sums)
{
    __shared__ T s_tmp[kScanBlock];
    const int64_t base = (int64_t)blockIdx.x * kScanItems + (int64_t)threadIdx.x * 8;
    T v[8], sum = 0;
    for (int j = 0; j < 8; j++) {
        v[j] = base + j < m ? buf[base + j] : T(0);
        sum += v[j];
    }
    T total;
    T run = block_exclusive_scan<T>(sum, s_tmp, &total);
    for (int j = 0; j < 8; j++) {
        if (base + j < m) buf[base + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

template <typename T>
__global__ __launch_bounds__(kScanBlock) void k_scan_sums(T* __restrict__ block_sums, int64_t nb, T* __restrict__ grand)
{
    __shared__ T s_tmp[kScanBlock];
    T carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += kScanBlock) {
        const int64_t b = b0 + (int64_t)threadIdx.x;
        const T v = b < nb ? block_sums[b] : T(0);
        T total;
        const T ex = block_exclusive_scan<T>(v, s_tmp, &total);
        if (b < nb) block_sums[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *grand = carry;
}

template <typename T>
__global__ __launch_bounds__(kScanBlock) void k_scan_add(T* __restrict__ buf, int64_t m, const T* __restrict__ block_sums,
                                                         const T* __restrict__ grand)
{
    const int64_t base = (int64_t)blockIdx.x * kScanItems + (int64_t)threadIdx.x * 8;
    const T add = block_sums[blockIdx.x];
    for (int j = 0; j < 8; j++)
        if (base + j < m) buf[base + j] += add;
    if (blockIdx.x == 0 && threadIdx.x == 0) buf[m] = *grand;
}

// Queues the scan of buf[0..m) on g.stream, the scan_blocks(m) + 1 values of its scratch taken from the stream-ordered pool and
// returned to it: SDFK_OK, or the failure as "<who>: <error string>".
template <typename T>
inline int scan(T* buf, int64_t m, const char* who)
{
    const int64_t nb = scan_blocks(m);
    T* aux = nullptr;   // the block totals, then the grand total
    if (int r = dev_alloc((void**)&aux, (size_t)(nb + 1) * sizeof(T))) return r;
    hipLaunchKernelGGL(k_scan_blocks<T>, dim3((unsigned)nb), dim3(kScanBlock), 0, g.stream, buf, m, aux);
    hipLaunchKernelGGL(k_scan_sums<T>, dim3(1), dim3(kScanBlock), 0, g.stream, aux, nb, aux + nb);
    hipLaunchKernelGGL(k_scan_add<T>, dim3((unsigned)nb), dim3(kScanBlock), 0, g.stream, buf, m, aux, aux + nb);
    dev_free(aux);   // (stream-ordered pool)
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SDFK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return SDFK_OK;
}

}  // namespace sdfk_scan
