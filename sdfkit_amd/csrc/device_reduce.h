// device_reduce.h -- the fixed-order block sum of the f64 reductions (lib_points.hip: ICP; lib_points_filter.hip: the outlier
// statistics): K doubles per thread through a halving tree in LDS, so that the result depends on the block's values and on nothing
// else -- no atomics, bitwise reproducible.  Blocks of kReduceBlock threads.
#pragma once
#include <hip/hip_runtime.h>

namespace sdfk_reduce {

constexpr int kReduceBlock = 256;

// s[t] += s[t + o] for t < o, o = 128, 64, ..., 1; every thread gets the block's totals
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

}  // namespace sdfk_reduce
