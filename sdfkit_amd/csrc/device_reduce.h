// device_reduce.h -- the fixed-order two-level f64 reduction of the KdTree family (lib_points.hip: ICP, both metrics;
// lib_points_filter.hip: the outlier statistics): no atomics, bitwise reproducible, the result a function of the values and of n.
// The order, stated here once (include/sdfkit_hip.h publishes it; tests/points_model.py reduce_fixed restates it):
//   first level   a grid of kReduceBlocks blocks of kReduceBlock threads; every thread starts each of its K accumulators at 0.0 and
//                 adds its items i = block * 256 + thread, then + 65536, ... in ascending i; the block's threads are summed by a tree
//                 that halves from 128 (s[t] += s[t + o] for t < o, o = 128, 64, ..., 1); the kernel writes the block's partial.
//   second level  one block (or every block alike): thread t adds partials t, t + 256, ... to a 0.0 of its own, then the same tree.
#pragma once
#include <hip/hip_runtime.h>

namespace sdfk_reduce {

constexpr int kReduceBlock = 256;
constexpr int kReduceBlocks = 256;   // a fixed grid: the summation order depends on n only

// the tree: every thread gets the block's totals of its K values (s: K rows of LDS)
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*s)[kReduceBlock])
{
#pragma unroll
    for (int j = 0; j < K; j++) s[j][threadIdx.x] = v[j];
    __syncthreads();
    for (int o = kReduceBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int j = 0; j < K; j++) s[j][threadIdx.x] += s[j][threadIdx.x + o];
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < K; j++) v[j] = s[j][0];
}

// the first level up to the tree: v = 0.0, then item(i, v) for the thread's items of [0, n) in ascending i
template <int K, class F>
__device__ __forceinline__ void grid_accumulate(int64_t n, double (&v)[K], F&& item)
{
#pragma unroll
    for (int j = 0; j < K; j++) v[j] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kReduceBlock + threadIdx.x; i < n; i += (int64_t)kReduceBlocks * kReduceBlock) item(i, v);
}

// the first level: -> v, the block's partial, in every thread
template <int K, class F>
__device__ __forceinline__ void grid_sum(int64_t n, double (&v)[K], double (*s)[kReduceBlock], F&& item)
{
    grid_accumulate(n, v, item);
    block_sum(v, s);
}

// the second level: columns off .. off + K - 1 of the kReduceBlocks partials -> out, in every thread
template <int K, int STRIDE>
__device__ __forceinline__ void sum_partials(const double (*part)[STRIDE], int off, double (&out)[K], double (*s)[kReduceBlock])
{
#pragma unroll
    for (int j = 0; j < K; j++) out[j] = 0.0;
    for (int b = threadIdx.x; b < kReduceBlocks; b += kReduceBlock)
#pragma unroll
        for (int j = 0; j < K; j++) out[j] += part[b][off + j];
    block_sum(out, s);
}

// the launch of a first-level kernel: the grid its stride assumes
template <class... P, class... A>
inline void launch_grid_sum(void (*kernel)(P...), hipStream_t stream, A... args)
{
    hipLaunchKernelGGL(kernel, dim3(kReduceBlocks), dim3(kReduceBlock), 0, stream, args...);
}

}  // namespace sdfk_reduce
