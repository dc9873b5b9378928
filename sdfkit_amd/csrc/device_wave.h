// device_wave.h -- what a kernel's lanes count with: the sum of a value over the wave, that sum added to a device word by one
// atomic per wave, and the number of lanes for which a flag holds.  Every lane of the wave calls these (the shuffle, the ballot): a
// lane with nothing to add passes 0 / false and leaves the kernel after the call, not before it.  Waves are 64 lanes wide and a
// block is a whole number of them, so lane 0 of a wave is (threadIdx.x & 63) == 0.  hipcc only.
#pragma once
#include <hip/hip_runtime.h>

// the sum of v over the wave; lane 0 holds it (the other lanes hold partial sums)
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// total += the wave's sum of n: one atomic per wave, none for a sum of zero.  A null total (uniform over the wave): nothing is counted.
__device__ __forceinline__ void wave_add(unsigned long long* total, unsigned long long n)
{
    if (!total) return;
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(total, n);
}

// the number of the wave's lanes whose flag is set, in every lane
__device__ __forceinline__ unsigned wave_count(bool flag) { return (unsigned)__popcll(__ballot(flag)); }
