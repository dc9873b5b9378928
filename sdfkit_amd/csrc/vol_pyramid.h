// vol_pyramid.h -- the min/max pyramid of one channel of a bound volume (sdfk_program_create_bound, SdfkVol::pyr / lev / nlev in
// sample_codegen.h): what iv_vox_box of the generated source reads.  Written once, here: lib_jit.hip's bind_volumes lays the
// snapshot out and calls these, and tests/test_gpu_intervals.py builds pyramids with the same code in a probe of its own.
// Needs hip/hip_runtime.h only.  Level L >= 1 has ((n + 2^L - 1) >> L) cells per axis, (lo, hi) per cell, at cell offset lev[L].
#pragma once
#include <hip/hip_runtime.h>

namespace {
__host__ __device__ inline bool finite_f(float v) { return v - v == 0.0f; }
// level 1 of a channel's pyramid from the voxels: cell c covers voxels [2c, 2c + 1] per axis (clipped); NaN when one is not finite
__global__ void k_vol_pyr_base(const float* __restrict__ src, int stride, int nx, int ny, int nz, int pitch, int cx, int cy, int cz,
                               float* __restrict__ out)
{
    const long total = (long)cx * cy * cz;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < total; c += (long)gridDim.x * 256) {
        const int k = (int)(c % cz);
        const long t = c / cz;
        const int j = (int)(t % cy), i = (int)(t / cy);
        float lo = __builtin_inff(), hi = -__builtin_inff();
        bool bad = false;
        for (int q = 0; q < 8; q++) {
            const int x = 2 * i + (q & 1), y = 2 * j + ((q >> 1) & 1), z = 2 * k + (q >> 2);
            if (x >= nx || y >= ny || z >= nz) continue;
            const float v = src[(((long)x * ny + y) * pitch + z) * stride];
            bad |= !finite_f(v);
            lo = __builtin_elementwise_minimum(lo, v);
            hi = __builtin_elementwise_maximum(hi, v);
        }
        out[2 * c] = bad ? __builtin_nanf("") : lo;
        out[2 * c + 1] = bad ? __builtin_nanf("") : hi;
    }
}
// level L + 1 from level L: minimum / maximum of up to 8 cells (IEEE 754:2019: a poisoned cell poisons its parent)
__global__ void k_vol_pyr_up(const float* __restrict__ in, int nx, int ny, int nz, float* __restrict__ out, int cx, int cy, int cz)
{
    const long total = (long)cx * cy * cz;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < total; c += (long)gridDim.x * 256) {
        const int k = (int)(c % cz);
        const long t = c / cz;
        const int j = (int)(t % cy), i = (int)(t / cy);
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (int q = 0; q < 8; q++) {
            const int x = 2 * i + (q & 1), y = 2 * j + ((q >> 1) & 1), z = 2 * k + (q >> 2);
            if (x >= nx || y >= ny || z >= nz) continue;
            const long e = ((long)x * ny + y) * nz + z;
            lo = __builtin_elementwise_minimum(lo, in[2 * e]);
            hi = __builtin_elementwise_maximum(hi, in[2 * e + 1]);
        }
        out[2 * c] = lo;
        out[2 * c + 1] = hi;
    }
}
inline int cells(int n, int L) { return (int)(((long)n + (1l << L) - 1) >> L); }
// the top level (one cell; 0: a single voxel, no pyramid) and the cell offsets lev[1 .. top] of a volume of n[0] x n[1] x n[2]
// voxels (lev[0] is not touched); returns the cells of all levels together
inline long long vol_pyr_levels(const int n[3], int* nlev, long long* lev)
{
    int top = 0;
    for (int a = 0; a < 3; a++)
        while ((1l << top) < n[a]) top++;
    *nlev = top;
    long long cells_so_far = 0;
    for (int L = 1; L <= top; L++) {
        lev[L] = cells_so_far;
        cells_so_far += (long long)cells(n[0], L) * cells(n[1], L) * cells(n[2], L);
    }
    return cells_so_far;
}
// blocks of 256 for nc cells: at least one, at most 256 * 8 (lib_internal.h's grid_for with its defaults); the kernels stride
inline int vol_pyr_grid(size_t nc)
{
    size_t b = (nc + 255) / 256;
    if (b < 1) b = 1;
    if (b > 256 * 8) b = 256 * 8;
    return (int)b;
}
// levels 1 .. nlev of one channel into P, on `stream`: src is the channel's first value (voxel i at src[i * stride], rows of `pitch`)
inline hipError_t vol_pyr_build(const float* src, int stride, const int n[3], int pitch, int nlev, const long long* lev, float* P,
                                hipStream_t stream)
{
    for (int L = 1; L <= nlev; L++) {
        const int cx = cells(n[0], L), cy = cells(n[1], L), cz = cells(n[2], L);
        const size_t nc = (size_t)cx * cy * cz;
        if (L == 1)
            hipLaunchKernelGGL(k_vol_pyr_base, dim3(vol_pyr_grid(nc)), dim3(256), 0, stream, src, stride, n[0], n[1], n[2], pitch, cx, cy, cz,
                               P + 2 * lev[1]);
        else
            hipLaunchKernelGGL(k_vol_pyr_up, dim3(vol_pyr_grid(nc)), dim3(256), 0, stream, P + 2 * lev[L - 1], cells(n[0], L - 1),
                               cells(n[1], L - 1), cells(n[2], L - 1), P + 2 * lev[L], cx, cy, cz);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}
}  // namespace
