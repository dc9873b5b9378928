// trimesh_sample.h -- the arithmetic of sdfk_trimesh_sample (lib_trimesh.hip: points sampled on a triangle mesh in proportion to
// area): the triangle weights, the stateless draws, the pick of a triangle from the integer prefix sums (plain and stratified),
// the fold of two draws into barycentric weights and the outputs of one sample.  Plain C++ outside hipcc, so that
// tests/cpp/mesh_sample_host.cpp runs exactly the code the kernels run.  Compiled with -ffp-contract=off everywhere: no
// expression below may be fused.  Everything that is accumulated is an integer: nothing depends on a summation order.
#pragma once
#include <cstdint>

#include "trimesh_sdf.h"

namespace sdfk_trimesh_smp {

using sdfk_trimesh_sdf::blend_colour;
using sdfk_trimesh_sdf::sq3;

constexpr uint64_t kOne53 = uint64_t(1) << 53;

// n = (b - a) x (c - a) in binary64 (each product rounded, then one subtraction); returns A2 = |n|^2 (sq3's order), four times
// the squared area.  Finite f32 vertices cannot make it overflow or NaN.
SDFK_TRI_HD inline double area2(const float a[3], const float b[3], const float c[3], double n[3])
{
    const double e1[3] = {(double)b[0] - (double)a[0], (double)b[1] - (double)a[1], (double)b[2] - (double)a[2]};
    const double e2[3] = {(double)c[0] - (double)a[0], (double)c[1] - (double)a[1], (double)c[2] - (double)a[2]};
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    return sq3(n);
}

// The integer weight of a triangle: its area over the largest one, in units of 2^-32, truncated (a2max > 0).  <= 2^32; 0 for
// an area below 2^-32 of the largest: such a triangle is never sampled.
SDFK_TRI_HD inline uint64_t weight(double a2, double a2max) { return (uint64_t)(__builtin_sqrt(a2 / a2max) * 4294967296.0); }

SDFK_TRI_HD inline uint64_t splitmix(uint64_t z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// draw j (0, 1, 2) of sample s: no state is carried from one sample to the next
SDFK_TRI_HD inline uint64_t draw(uint64_t seed, uint64_t s, int j) { return splitmix(seed + (3 * s + (uint64_t)j + 1) * 0x9E3779B97F4A7C15ull); }

// the high 64 bits of a * b
SDFK_TRI_HD inline uint64_t mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// floor(s total / n) for 0 <= s <= n < 2^31 and total < 2^63, every product within 64 bits
SDFK_TRI_HD inline uint64_t stratum(uint64_t s, uint64_t total, uint64_t n) { return (total / n) * s + ((total % n) * s) / n; }

// r in [0, total): uniform over the whole (plain) or over stratum s of n (stratified; an empty stratum gives its own start)
SDFK_TRI_HD inline uint64_t pick(uint64_t h0, uint64_t s, uint64_t n, uint64_t total, bool stratified)
{
    if (!stratified) return mulhi64(h0, total);
    const uint64_t lo = stratum(s, total, n);
    return lo + mulhi64(h0, stratum(s + 1, total, n) - lo);
}

// The triangle t with W[t] <= r < W[t + 1], W the exclusive prefix sums of the nt weights (W[nt] = total > r): triangles of
// weight zero have empty intervals and are never found.
SDFK_TRI_HD inline int64_t find_triangle(const unsigned long long* W, int64_t nt, uint64_t r)
{
    int64_t lo = 0, hi = nt - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (W[mid + 1] <= r) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Two draws folded into the triangle: k1, k2 their top 53 bits, reflected when they leave it; k0 = 2^53 - k1 - k2 >= 0.  The
// weights k * 2^-53 are exact in binary64 and sum to 1 exactly.
SDFK_TRI_HD inline void fold(uint64_t h1, uint64_t h2, double w[3])
{
    uint64_t k1 = h1 >> 11, k2 = h2 >> 11;
    if (k1 + k2 > kOne53) { k1 = kOne53 - k1; k2 = kOne53 - k2; }
    const uint64_t k0 = kOne53 - k1 - k2;
    w[0] = (double)k0 * 0x1p-53; w[1] = (double)k1 * 0x1p-53; w[2] = (double)k2 * 0x1p-53;
}

struct Sample {
    float point[3];     // (float)((w0 a + w1 b) + w2 c), binary64 inside
    float normal[3];    // (float)(n / sqrt(A2)): the unit face normal of the winding (b - a) x (c - a)
    float weights[3];   // (float)w: the weights blend_colour uses
    double w[3];
};

// The outputs of one sample on triangle (a, b, c), which has an area (A2 > 0).
SDFK_TRI_HD inline Sample sample_on(const float a[3], const float b[3], const float c[3], uint64_t h1, uint64_t h2)
{
    Sample S;
    fold(h1, h2, S.w);
    double n[3];
    const double len = __builtin_sqrt(area2(a, b, c, n));
    for (int k = 0; k < 3; k++) {
        S.point[k] = (float)((S.w[0] * (double)a[k] + S.w[1] * (double)b[k]) + S.w[2] * (double)c[k]);
        S.normal[k] = (float)(n[k] / len);
        S.weights[k] = (float)S.w[k];
    }
    return S;
}

}  // namespace sdfk_trimesh_smp
