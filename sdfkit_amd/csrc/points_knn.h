// points_knn.h -- the arithmetic of the KdTree's k-nearest and radius queries (lib_points_knn.hip), written once for the device
// and the host: the packed (d2, index) key, the bounded candidate lists, the radius predicate and the stopping rule of the shell
// walk.  Plain C++ outside hipcc, so that tests/cpp/points_knn_host.cpp checks it as the kernels run it.
//
// Order (include/sdfkit_hip.h, "k nearest / within a radius"): static points are ordered by (d2, index), d2 = (dx*dx + dy*dy) + dz*dz
// in binary32 without FMA, the smaller d2 first, equal d2 to the lower index.  d2 >= 0, so its bits order as an unsigned integer and
// key = bits(d2) << 32 | index orders the pair with one 64-bit compare.  A point counts iff d2 < +inf (sqrtf(d2) < FLT_MAX), i.e.
// key < kKeyInf.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SDFK_KNN_HD __host__ __device__ __forceinline__
#else
#define SDFK_KNN_HD inline
#endif

namespace sdfk_knn {

constexpr int kMaxK = 64;
constexpr uint64_t kKeyInf = uint64_t(0x7f800000u) << 32;   // (d2 = +inf, index 0): above every counting key, the empty slot

SDFK_KNN_HD uint32_t f32_bits(float x)
{
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}
SDFK_KNN_HD float bits_f32(uint32_t u)
{
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}
SDFK_KNN_HD uint64_t pack_key(float d2, int32_t index) { return (uint64_t)f32_bits(d2) << 32 | (uint32_t)index; }
SDFK_KNN_HD float key_d2(uint64_t key) { return bits_f32((uint32_t)(key >> 32)); }
SDFK_KNN_HD int32_t key_index(uint64_t key) { return (int32_t)(uint32_t)key; }
SDFK_KNN_HD float sqrt_rn(float x) { return (float)__builtin_sqrt((double)x); }   // (correctly rounded sqrtf: 53 >= 2 * 24 + 2)
SDFK_KNN_HD float dist2(float qx, float qy, float qz, float px, float py, float pz)
{
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
#else
    return (dx * dx + dy * dy) + dz * dz;   // (built with -ffp-contract=off)
#endif
}

// ---- within a radius ----------------------------------------------------------------------------------------------------------
// A counting point is within r iff sqrtf(d2) <= r.  sqrtf is monotone, so that is d2 <= radius_d2_bound(r): the largest finite d2
// whose correctly rounded root does not exceed r (r >= 0 or +inf; FLT_MAX for every r from sqrtf(FLT_MAX) on: every counting point).
SDFK_KNN_HD float radius_d2_bound(float r)
{
    const double rr = (double)r * (double)r;
    float t = rr >= (double)FLT_MAX ? FLT_MAX : (float)rr;
    while (t > 0.0f && sqrt_rn(t) > r) t = bits_f32(f32_bits(t) - 1u);
    while (t < FLT_MAX && sqrt_rn(bits_f32(f32_bits(t) + 1u)) <= r) t = bits_f32(f32_bits(t) + 1u);
    return t;
}
SDFK_KNN_HD bool within(float d2, float d2_bound) { return d2 <= d2_bound; }   // (false for +inf and NaN: the bound is finite)
SDFK_KNN_HD bool radius_is_valid(float r) { return r >= 0.0f; }                // (false for NaN and negative radii)

// ---- the stopping rule ---------------------------------------------------------------------------------------------------------
// lb2: the conservative lower bound of d2 over every unvisited cell (points_walk.h's lb_sq).  The walk stops once that bound, with
// the search's 2^-18 margin, exceeds both what the list would still take (the d2 of its worst key; +inf until k are held) and the
// radius bound.  Strictly: a cell at exactly the worst d2 may hold an equal d2 with a lower index.
SDFK_KNN_HD bool walk_done(float lb2, uint64_t worst, float d2_bound) { return lb2 * (1.0f - 0x1p-18f) > fminf(key_d2(worst), d2_bound); }

// capacity tier of k (1 <= k <= kMaxK): the kernels are instantiated per tier
SDFK_KNN_HD int tier_of(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

// ---- binary max-heap over any storage with get(i) / set(i, key) ---------------------------------------------------------------
template <class S>
SDFK_KNN_HD void heap_sift_down(S& s, int n, int i, uint64_t key)   // places `key` at or below i
{
    for (;;) {
        int c = 2 * i + 1;
        if (c >= n) break;
        uint64_t ck = s.get(c);
        if (c + 1 < n) {
            const uint64_t rk = s.get(c + 1);
            if (rk > ck) { ck = rk; c++; }
        }
        if (ck <= key) break;
        s.set(i, ck);
        i = c;
    }
    s.set(i, key);
}
template <class S>
SDFK_KNN_HD void heap_sift_up(S& s, int i, uint64_t key)   // places `key` at or above i
{
    while (i > 0) {
        const int p = (i - 1) >> 1;
        const uint64_t pk = s.get(p);
        if (pk >= key) break;
        s.set(i, pk);
        i = p;
    }
    s.set(i, key);
}
template <class S>
SDFK_KNN_HD void heap_make(S& s, int n)
{
    for (int i = n / 2 - 1; i >= 0; i--) heap_sift_down(s, n, i, s.get(i));
}
// a max-heap of n keys -> ascending order, in place
template <class S>
SDFK_KNN_HD void heap_sort(S& s, int n)
{
    for (int m = n - 1; m > 0; m--) {
        const uint64_t last = s.get(m);
        s.set(m, s.get(0));
        heap_sift_down(s, m, 0, last);
    }
}

// ---- bounded candidate lists: the k least keys seen ------------------------------------------------------------------------------
// Both kinds: init(k); `worst()` is the key a candidate has to be BELOW to enter (kKeyInf until k are held); insert(key) is called
// with key < worst() only; finish() orders the list; at(i) is then the i-th least key, kKeyInf from count() on.

// (a) a max-heap in indexed storage (the kernels: LDS, slot-major)
template <class S>
struct HeapList {
    S s;
    int n, k;
    uint64_t w;
    SDFK_KNN_HD void init(int k_) { n = 0; k = k_; w = kKeyInf; }
    SDFK_KNN_HD uint64_t worst() const { return w; }
    SDFK_KNN_HD void insert(uint64_t key)
    {
        if (n < k) {
            heap_sift_up(s, n, key);
            n++;
            if (n == k) w = s.get(0);
        } else {
            heap_sift_down(s, n, 0, key);
            w = s.get(0);
        }
    }
    SDFK_KNN_HD void finish() { heap_sort(s, n); }
    SDFK_KNN_HD int count() const { return n; }
    SDFK_KNN_HD uint64_t at(int i) const { return i < n ? s.get(i) : kKeyInf; }
};

// (b) a sorted array of CAP keys with constant indices only (the kernels: registers); at(i) wants a constant i (unrolled loops)
template <int CAP>
struct SortedList {
    uint64_t v[CAP];
    int k;
    uint64_t w;
    SDFK_KNN_HD void init(int k_)
    {
        k = k_;
        w = kKeyInf;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < CAP; i++) v[i] = kKeyInf;
    }
    SDFK_KNN_HD uint64_t worst() const { return w; }
    SDFK_KNN_HD void insert(uint64_t key)
    {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = CAP - 1; i > 0; i--) v[i] = key < v[i - 1] ? v[i - 1] : (key < v[i] ? key : v[i]);
        v[0] = key < v[0] ? key : v[0];
        uint64_t kth = v[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 1; i < CAP; i++) kth = i < k ? v[i] : kth;
        w = kth;
    }
    SDFK_KNN_HD void finish() {}
    SDFK_KNN_HD int count() const
    {
        int c = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < CAP; i++) c += (i < k && v[i] < kKeyInf) ? 1 : 0;
        return c;
    }
    SDFK_KNN_HD uint64_t at(int i) const { return i < k ? v[i] : kKeyInf; }
};

}  // namespace sdfk_knn
