// points_filter.h -- the arithmetic of the KdTree's two filters (lib_points_filter.hip), written once for the device and the host:
// the voxel of a coordinate, the range check and the packed key of sdfk_points_voxel_downsample, its chunked centroid sum, and the
// mean / threshold / keep rule of sdfk_points_outliers.  Plain C++ outside hipcc, so that tests/cpp/points_filter_host.cpp checks
// it as the kernels run it.  Contract: include/sdfkit_hip.h, "Point clouds: filters".  One rounding per written operation
// (-ffp-contract=off), binary64 from the f32 inputs.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SDFK_FILTER_HD __host__ __device__ __forceinline__
#else
#define SDFK_FILTER_HD inline
#endif

namespace sdfk_filter {

constexpr int kChunk = 32;       // members of a chunk of the centroid sum
constexpr int kAxisBits = 21;    // bits of an axis in the packed key
constexpr double kAxisSpan = 2097152.0;   // 2^21: voxels an axis may span

// ---- voxel downsample ----------------------------------------------------------------------------------------------------------
// The voxel of a coordinate along one axis, as an integer-valued binary64: floor((p - o) / size).  Monotone in p.
SDFK_FILTER_HD double voxel_of(float p, float o, float size) { return __builtin_floor(((double)p - (double)o) / (double)size); }

SDFK_FILTER_HD bool size_is_valid(float size) { return size > 0.0f && size < INFINITY; }   // (false for NaN)
SDFK_FILTER_HD bool origin_is_valid(const float o[3]) { return fabsf(o[0]) < INFINITY && fabsf(o[1]) < INFINITY && fabsf(o[2]) < INFINITY; }

// an axis whose voxels run from kmin to kmax is accepted iff kmax - kmin < 2^21 (the difference of two integer-valued doubles
// that close is exact; a larger one, exact or not, is refused)
SDFK_FILTER_HD bool span_is_valid(double kmin, double kmax) { return kmax - kmin < kAxisSpan; }

// bits the offsets 0 .. kmax - kmin of an axis need (0: one voxel)
SDFK_FILTER_HD int span_bits(double kmin, double kmax)
{
    uint64_t d = (uint64_t)(kmax - kmin);
    int b = 0;
    while (d) { b++; d >>= 1; }
    return b;
}

struct Lattice {
    float origin[3];
    float size;
    double kmin[3];
};

SDFK_FILTER_HD uint64_t voxel_key(const Lattice& L, float x, float y, float z)
{
    const uint64_t kx = (uint64_t)(voxel_of(x, L.origin[0], L.size) - L.kmin[0]);
    const uint64_t ky = (uint64_t)(voxel_of(y, L.origin[1], L.size) - L.kmin[1]);
    const uint64_t kz = (uint64_t)(voxel_of(z, L.origin[2], L.size) - L.kmin[2]);
    return kz << (2 * kAxisBits) | ky << kAxisBits | kx;
}

// the 8-bit digits of the packed key that can be non-zero, as a mask of passes (bit d: bits 8d .. 8d + 7)
SDFK_FILTER_HD unsigned digit_mask(const int bits[3])
{
    unsigned m = 0;
    for (int a = 0; a < 3; a++)
        for (int b = a * kAxisBits; b < a * kAxisBits + bits[a]; b++) m |= 1u << (b >> 3);
    return m;
}

// The centroid sum of a voxel, per axis: its members in ascending index are cut into chunks of kChunk (the last may be short); a
// chunk is a Sum3 that takes its members in order (add_point: widened first), the voxel's total a Sum3 that takes the chunk sums in
// order (add_sum).  Both start at +0.0.
struct Sum3 {
    double v[3] = {0.0, 0.0, 0.0};
    SDFK_FILTER_HD void add_point(float x, float y, float z)
    {
        v[0] = v[0] + (double)x;
        v[1] = v[1] + (double)y;
        v[2] = v[2] + (double)z;
    }
    SDFK_FILTER_HD void add_sum(const double s[3])
    {
        v[0] = v[0] + s[0];
        v[1] = v[1] + s[1];
        v[2] = v[2] + s[2];
    }
};
SDFK_FILTER_HD float centroid_of(double total, int64_t count) { return (float)(total / (double)count); }
SDFK_FILTER_HD int64_t chunks_of(int64_t count) { return (count + kChunk - 1) / kChunk; }

// ---- statistical outliers ------------------------------------------------------------------------------------------------------
// mean_i from the sum of the row's distances without its first entry; found < 2: isolated, +inf
SDFK_FILTER_HD double row_mean(double sum_rest, int found) { return found < 2 ? (double)INFINITY : sum_rest / (double)(found - 1); }
SDFK_FILTER_HD bool is_isolated(double mean) { return !(mean < (double)INFINITY); }

// finite and not negative (false for NaN): +inf times a sigma of 0 would make the threshold a NaN, under which nothing is kept
SDFK_FILTER_HD bool ratio_is_valid(float std_ratio) { return std_ratio >= 0.0f && std_ratio < INFINITY; }

struct Threshold {
    double mu, sigma, thr;
};
// sum: the sum of the c means; sqsum: the sum of (mean_i - mu)^2, mu from this function with sqsum = 0
SDFK_FILTER_HD Threshold threshold_of(double sum, double sqsum, double c, float std_ratio)
{
    Threshold t{0.0, 0.0, 0.0};
    if (!(c > 0.0)) return t;
    t.mu = sum / c;
    t.sigma = __builtin_sqrt(sqsum / c);
    t.thr = t.mu + (double)std_ratio * t.sigma;
    return t;
}
SDFK_FILTER_HD bool is_kept(double mean, double thr) { return !is_isolated(mean) && mean <= thr; }

}  // namespace sdfk_filter
