// lib_pointcloud.hip -- the KdTree's point cloud as geometry: normals (sdfk_points_normals*), signed distance volumes
// (sdfk_points_to_volume*) and per-point colours at queries and in volumes (sdfk_points_blend_colors*,
// sdfk_points_to_volume_colors*).  Contract: include/sdfkit_hip.h, "Point clouds: normals and volumes" and "Point clouds:
// colours"; the arithmetic (covariance, Jacobi eigenvectors, orientation, the blend of tangent-plane distances, the fill of one
// line): points_normals.h, (the blend of colours): points_color.h, both checked on the host; the walk, the tiers, the bounded
// lists and the profiled launch (walk_launch): points_walk.h / points_knn.h, shared with every query of the KdTree.
//
//   k_pc_normals<CAP>   one lane per static point: its k nearest (itself included) exactly as k_pts_knn<CAP> finds them -- CAP = 8
//                       in registers, 16 / 32 / 64 a heap in LDS, one wave per block --, then two passes over the list (mean,
//                       covariance; the neighbours' coordinates gathered from the insertion-order array) and the binary64 eigen
//                       step, all in the same lane.
//   k_pc_volume<CAP, COLOR>  one lane per voxel: the k nearest of the cell centre, the blend over them (coordinates and normals
//                       gathered), the value and a sign byte (0: unknown).  COLOR: the same list feeds the colour blend as well
//                       (colours gathered; every voxel's colour is written, zero where nothing was found); without it the kernel is
//                       what it was before colours.
//   k_pc_colors<CAP>    one lane per query: its k nearest, the colour blend over them, the colour and the number found.
//   k_pc_fill<AXIS>     one lane per line of sign bytes along z, then y, then x: unknown voxels take the sign carried along the
//                       line and the value +-max_distance.  Lines along z are walked by neighbouring lanes nz bytes apart
//                       (uncoalesced; the array is one byte per voxel and each line stays in cache), the other two coalesce.
// Host side: the volume's scratch (sign bytes, the known count) and the host forms' device copies are held in a Staged (device_stage.h).
#include "lib_internal.h"
#include "points_color.h"
#include "points_knn.h"
#include "points_normals.h"
#include "points_set.h"
#include "points_walk.h"

#include <cfloat>

namespace {

using namespace sdfk_walk;
using namespace sdfk_pc;

// ---- normals -------------------------------------------------------------------------------------------------------------------
struct NormalsArgs {
    const float* xyz;        // the static points, insertion order
    int64_t n;
    int k;
    float d2_bound;
    const float* view;       // n_view x 3
    int64_t n_view;          // 0: none, 1: one for all, n: one per point
    float* normals;          // n x 3, may be null
    float* variation;        // n, may be null
    unsigned long long* candidates;
};

template <int CAP>
__global__ __launch_bounds__(block_of<CAP>()) void k_pc_normals(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                                 NormalsArgs A)
{
    __shared__ uint64_t s_keys[lds_keys<CAP>()];
    const int64_t t = (int64_t)blockIdx.x * block_of<CAP>() + threadIdx.x;
    const Query q = load_query(A.xyz, t, A.n);
    Neighbours<CAP> nb;
    const unsigned long long ncand = nb.collect(sorted, starts, G, q, A.k, A.d2_bound, s_keys);
    if (t < A.n) {
        const float pi[3] = {q.x, q.y, q.z};
        Mean mean;
        nb.each([&](uint64_t key) {
            float p[3];
            load3(A.xyz, key_index(key), p);
            mean.add(p, pi);
            return true;
        });
        if (nb.m > 0) mean.finish(nb.m);
        Cov C;
        nb.each([&](uint64_t key) {
            float p[3];
            load3(A.xyz, key_index(key), p);
            C.add(p, pi, mean);
            return true;
        });
        float w[3] = {0.0f, 0.0f, 0.0f};
        if (A.n_view) load3(A.view, A.n_view == 1 ? 0 : t, w);
        float nrm[3], var;
        normal_of(C, nb.m, pi, A.n_view != 0, w, nrm, &var);
        if (A.normals) { A.normals[3 * t] = nrm[0]; A.normals[3 * t + 1] = nrm[1]; A.normals[3 * t + 2] = nrm[2]; }
        if (A.variation) A.variation[t] = var;
    }
    wave_add(A.candidates, ncand);
}

// ---- the volume ----------------------------------------------------------------------------------------------------------------
struct VolumeArgs {
    const float* xyz;
    const float* normals;    // one per static point
    float* values;
    signed char* sgn;        // nx * ny * nz (unpadded rows): 0 unknown, +-1
    int nx, ny, nz, pitch, z0;
    float mx, my, mz, dx, dy, dz;
    int k;
    float d2_bound, max_distance;
    unsigned long long* known;        // null: not counted
    unsigned long long* candidates;
    const float* colors3;    // COLOR: one colour per static point
    float* colors_out;       // COLOR: the volume's colours, rows padded as the values'
};

template <int CAP, bool COLOR>
__global__ __launch_bounds__(block_of<CAP>()) void k_pc_volume(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                                VolumeArgs A)
{
    __shared__ uint64_t s_keys[lds_keys<CAP>()];
    const int64_t n = (int64_t)A.nx * A.ny * A.nz;
    const int64_t g0 = (int64_t)blockIdx.x * block_of<CAP>() + threadIdx.x;
    const bool active = g0 < n;
    const int64_t gidx = active ? g0 : 0;
    const int kz = (int)(gidx % A.nz);
    const int64_t row = gidx / A.nz;   // = i * ny + j
    const int j = (int)(row % A.ny), i = (int)(row / A.ny);
    // the cell centre, as sdfk_sample and sdfk_trimesh_to_volume place it
    const float x[3] = {A.mx + (float)i * A.dx, A.my + (float)j * A.dy, A.mz + (float)(A.z0 + kz) * A.dz};
    Query q{x[0], x[1], x[2], false};
    q.finite = active && isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
    Neighbours<CAP> nb;
    const unsigned long long ncand = nb.collect(sorted, starts, G, q, A.k, A.d2_bound, s_keys);
    bool known = false;
    if (active) {
        Blend b;
        sdfk_color::Blend cb;
        if (nb.m > 0) {
            const float h2 = cutoff_d2(nb.m, A.k, key_d2(nb.last()), A.d2_bound);
            nb.each([&](uint64_t key) {
                float p[3], nr[3];
                load3(A.xyz, key_index(key), p);
                load3(A.normals, key_index(key), nr);
                b.add(x, p, nr, key_d2(key), h2);
                if constexpr (COLOR) {
                    float c[3];
                    load3(A.colors3, key_index(key), c);
                    cb.add(c, key_d2(key), h2);
                }
                return true;
            });
        }
        if constexpr (COLOR) {
            float rgb[3];
            cb.result(rgb);
            const size_t o = (size_t)row * A.pitch + kz;
            for (int a = 0; a < 3; a++) A.colors_out[3 * o + a] = rgb[a];
        }
        known = b.known();
        signed char s = 0;
        if (known) {
            const float v = b.value(A.max_distance);
            A.values[(size_t)row * A.pitch + kz] = v;
            s = (signed char)sign_of(v);
        }
        A.sgn[gidx] = s;
    }
    if (A.known) {
        const unsigned long long c = wave_count(known);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(A.known, c);
    }
    wave_add(A.candidates, ncand);
}

// One lane per line along AXIS (2: z, 1: y, 0: x).  LAST (the pass along x): a line without a sign means a volume without one,
// which becomes +max_distance.
template <int AXIS>
__global__ __launch_bounds__(kBlock) void k_pc_fill(signed char* __restrict__ sgn, float* __restrict__ values, int nx, int ny, int nz, int pitch,
                                                    float max_distance)
{
    const int64_t lines = AXIS == 2 ? (int64_t)nx * ny : AXIS == 1 ? (int64_t)nx * nz : (int64_t)ny * nz;
    const int64_t L = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (L >= lines) return;
    int64_t sbase, vbase;
    long long sstride, vstride;
    int len;
    if (AXIS == 2) {
        sbase = L * nz; vbase = L * pitch; sstride = 1; vstride = 1; len = nz;
    } else if (AXIS == 1) {
        const int64_t i = L / nz, k = L % nz;
        sbase = i * ny * nz + k; vbase = i * ny * pitch + k; sstride = nz; vstride = pitch; len = ny;
    } else {
        const int64_t j = L / nz, k = L % nz;
        sbase = j * nz + k; vbase = j * pitch + k; sstride = (long long)ny * nz; vstride = (long long)ny * pitch; len = nx;
    }
    float* val = values + vbase;
    const bool had = fill_line(sgn + sbase, len, sstride, [&](int i, int s) { val[(long long)i * vstride] = s < 0 ? -max_distance : max_distance; });
    if (AXIS == 0 && !had)
        for (int i = 0; i < len; i++) {
            sgn[sbase + (long long)i * sstride] = 1;
            val[(long long)i * vstride] = max_distance;
        }
}

// ---- colours at queries --------------------------------------------------------------------------------------------------------
struct ColorArgs {
    const float* colors3;    // one colour per static point, insertion order
    const float* queries;
    int64_t nq;
    int k;
    float d2_bound;
    float* colors_out;       // nq x 3, may be null
    int32_t* found;          // nq, may be null
    unsigned long long* candidates;
};

template <int CAP>
__global__ __launch_bounds__(block_of<CAP>()) void k_pc_colors(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                                ColorArgs A)
{
    __shared__ uint64_t s_keys[lds_keys<CAP>()];
    const int64_t t = (int64_t)blockIdx.x * block_of<CAP>() + threadIdx.x;
    const Query q = load_query(A.queries, t, A.nq);
    Neighbours<CAP> nb;
    const unsigned long long ncand = nb.collect(sorted, starts, G, q, A.k, A.d2_bound, s_keys);
    if (t < A.nq) {
        sdfk_color::Blend cb;
        if (nb.m > 0) {
            const float h2 = cutoff_d2(nb.m, A.k, key_d2(nb.last()), A.d2_bound);
            nb.each([&](uint64_t key) {
                float c[3];
                load3(A.colors3, key_index(key), c);
                cb.add(c, key_d2(key), h2);
                return true;
            });
        }
        if (A.colors_out) {
            float rgb[3];
            cb.result(rgb);
            A.colors_out[3 * t] = rgb[0]; A.colors_out[3 * t + 1] = rgb[1]; A.colors_out[3 * t + 2] = rgb[2];
        }
        if (A.found) A.found[t] = nb.m;
    }
    wave_add(A.candidates, ncand);
}

// ---- launches ----------------------------------------------------------------------------------------------------------------
int colors_launch(const sdfk_points* s, ColorArgs A)
{
    return walk_launch(s, A.nq, "k_pc_colors", "sdfk_points_blend_colors", [&](unsigned long long* counter) {
        A.candidates = counter;
        launch_tier(A.k, A.nq, [&](auto cap, dim3 grid, dim3 block) {
            hipLaunchKernelGGL(k_pc_colors<decltype(cap)::value>, grid, block, 0, g.stream, s->sorted, s->starts, s->G, A);
        });
    });
}

int check_colors(const sdfk_points* s, const void* colors3, const void* queries, int64_t n, int32_t k, float max_distance)
{
    static const char* who = "sdfk_points_blend_colors";
    if (int r = require_init()) return r;
    if (!s || !colors3 || n < 0 || (n > 0 && !queries)) return fail(SDFK_ERR_INVALID, "%s: null / negative argument", who);
    if (n >= (int64_t(1) << 32)) return fail(SDFK_ERR_INVALID, "%s: 2^32 queries or more", who);
    if (k < 1 || k > kMaxK) return fail(SDFK_ERR_INVALID, "%s: k = %d is outside [1, %d]", who, (int)k, kMaxK);
    if (!radius_is_valid(max_distance)) return fail(SDFK_ERR_INVALID, "%s: max_distance is negative or NaN", who);
    return SDFK_OK;
}

int normals_launch(const sdfk_points* s, int k, float d2_bound, const float* view_dev, int64_t n_view, float* normals_dev, float* variation_dev)
{
    return walk_launch(s, s->n, "k_pc_normals", "sdfk_points_normals", [&](unsigned long long* counter) {
        const NormalsArgs A{s->xyz, s->n, k, d2_bound, view_dev, n_view, normals_dev, variation_dev, counter};
        launch_tier(k, s->n, [&](auto cap, dim3 grid, dim3 block) {
            hipLaunchKernelGGL(k_pc_normals<decltype(cap)::value>, grid, block, 0, g.stream, s->sorted, s->starts, s->G, A);
        });
    });
}

int check_normals(const sdfk_points* s, int32_t k, float max_distance, const void* view, int64_t n_view)
{
    static const char* who = "sdfk_points_normals";
    if (int r = require_init()) return r;
    if (!s) return fail(SDFK_ERR_INVALID, "%s: null point set", who);
    if (k < kMinNormalK || k > kMaxK) return fail(SDFK_ERR_INVALID, "%s: k = %d is outside [%d, %d]", who, (int)k, kMinNormalK, kMaxK);
    if (!radius_is_valid(max_distance)) return fail(SDFK_ERR_INVALID, "%s: max_distance is negative or NaN", who);
    if (!(n_view == 0 || n_view == 1 || n_view == s->n) || (n_view > 0 && !view))
        return fail(SDFK_ERR_INVALID, "%s: viewpoints must be none, one, or one per static point", who);
    return SDFK_OK;
}

// colors_dev: null for the colourless call (the volume's colours stay), else one colour per static point and v has colour storage
int to_volume(const sdfk_points* s, const float* normals_dev, const float* colors_dev, sdfk_volume* v, int k, float max_distance, int64_t stats[4])
{
    const char* who = colors_dev ? "sdfk_points_to_volume_colors" : "sdfk_points_to_volume";
    resolve_dependents(v);   // (a queued mesh may still read the old values)
    volume_values_changed(v);
    float d[3], m[3], outside;
    grid_constants(v, d, m, &outside);
    const int64_t nvox = (int64_t)v->nx * v->ny * v->nz;
    Staged st;
    signed char* sgn = st.scratch<signed char>((size_t)nvox);
    unsigned long long* known = stats ? st.scratch<unsigned long long>(1) : nullptr;
    unsigned long long c = 0;
    if (stats) st.run([&] { return hipMemsetAsync(known, 0, sizeof(unsigned long long), g.stream); });
    st.run([&] {
        return walk_launch(s, nvox, "k_pc_volume", who, [&](unsigned long long* counter) {
            const VolumeArgs A{s->xyz, normals_dev, v->values, sgn, v->nx, v->ny, v->nz, v->pitch(), v->z0, m[0], m[1], m[2], d[0], d[1], d[2],
                               k, radius_d2_bound(max_distance), max_distance, known, counter, colors_dev, colors_dev ? v->colors : nullptr};
            launch_tier(k, nvox, [&](auto cap, dim3 grid, dim3 block) {
                if (colors_dev)
                    hipLaunchKernelGGL((k_pc_volume<decltype(cap)::value, true>), grid, block, 0, g.stream, s->sorted, s->starts, s->G, A);
                else
                    hipLaunchKernelGGL((k_pc_volume<decltype(cap)::value, false>), grid, block, 0, g.stream, s->sorted, s->starts, s->G, A);
            });
        });
    });
    st.run([&] {
        ProfScope ps("k_pc_fill");
        const int nx = v->nx, ny = v->ny, nz = v->nz, pitch = v->pitch();
        hipLaunchKernelGGL(k_pc_fill<2>, dim3(grid_of((int64_t)nx * ny, kBlock)), dim3(kBlock), 0, g.stream, sgn, v->values, nx, ny, nz, pitch, max_distance);
        hipLaunchKernelGGL(k_pc_fill<1>, dim3(grid_of((int64_t)nx * nz, kBlock)), dim3(kBlock), 0, g.stream, sgn, v->values, nx, ny, nz, pitch, max_distance);
        hipLaunchKernelGGL(k_pc_fill<0>, dim3(grid_of((int64_t)ny * nz, kBlock)), dim3(kBlock), 0, g.stream, sgn, v->values, nx, ny, nz, pitch, max_distance);
    });
    if (stats) st.read(&c, known, sizeof c);
    if (int r = st.finish(who, false)) return r;   // (no wait of its own: with stats the read above was one)
    if (stats) {
        stats[0] = (int64_t)c;
        stats[1] = nvox - (int64_t)c;
        stats[2] = g.prof_on ? s->last_candidates : 0;
        stats[3] = g.prof_on ? s->last_queries : 0;
    }
    return SDFK_OK;
}

int check_volume(const sdfk_points* s, const void* normals, const sdfk_volume* v, int32_t k, float max_distance,
                 const char* who = "sdfk_points_to_volume")
{
    if (int r = require_init()) return r;
    if (!s || !v || !normals) return fail(SDFK_ERR_INVALID, "%s: null argument", who);
    if (k < 1 || k > kMaxK) return fail(SDFK_ERR_INVALID, "%s: k = %d is outside [1, %d]", who, (int)k, kMaxK);
    if (!(max_distance > 0.0f)) return fail(SDFK_ERR_INVALID, "%s: max_distance must be > 0 (+inf: no band)", who);
    if (v->elided || !v->values) return fail(SDFK_ERR_INVALID, "%s: the volume has no storage", who);
    if (v->owner != s->owner) return fail(SDFK_ERR_INVALID, "%s: the volume belongs to another device context", who);
    return SDFK_OK;
}

int check_volume_colors(const sdfk_points* s, const void* normals, const void* colors3, const sdfk_volume* v, int32_t k, float max_distance)
{
    static const char* who = "sdfk_points_to_volume_colors";
    if (int r = check_volume(s, normals, v, k, max_distance, who)) return r;
    if (!colors3) return fail(SDFK_ERR_INVALID, "%s: null colours", who);
    if (!v->colors) return fail(SDFK_ERR_INVALID, "%s: the volume was created without colours", who);
    return SDFK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_points_normals_device(const sdfk_points* s, int32_t k, float max_distance, const void* viewpoints3_dev, int64_t n_viewpoints,
                                          void* normals3_dev, void* variation_dev)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_normals(s, k, max_distance, viewpoints3_dev, n_viewpoints)) return r;
    return normals_launch(s, k, radius_d2_bound(max_distance), (const float*)viewpoints3_dev, n_viewpoints, (float*)normals3_dev, (float*)variation_dev);
}

extern "C" int sdfk_points_normals(const sdfk_points* s, int32_t k, float max_distance, const float* viewpoints3, int64_t n_viewpoints, float* normals3,
                                   float* variation)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_normals(s, k, max_distance, viewpoints3, n_viewpoints)) return r;
    for (int64_t i = 0; i < 3 * n_viewpoints; i++)
        if (!std::isfinite(viewpoints3[i])) return fail(SDFK_ERR_INVALID, "sdfk_points_normals: viewpoint %lld has a NaN or infinite coordinate", (long long)(i / 3));
    Staged st;
    const float* vd = st.in(viewpoints3, (size_t)n_viewpoints * 3);
    float* nd = st.out(normals3, (size_t)s->n * 3);
    float* wd = st.out(variation, (size_t)s->n);
    st.run([&] { return normals_launch(s, k, radius_d2_bound(max_distance), vd, n_viewpoints, nd, wd); });
    return st.finish("sdfk_points_normals");
}

extern "C" int sdfk_points_to_volume_device(const sdfk_points* s, const void* normals3_dev, sdfk_volume* v, int32_t k, float max_distance,
                                            int64_t stats[4])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_volume(s, normals3_dev, v, k, max_distance)) return r;
    return to_volume(s, (const float*)normals3_dev, nullptr, v, k, max_distance, stats);
}

extern "C" int sdfk_points_to_volume(const sdfk_points* s, const float* normals3, sdfk_volume* v, int32_t k, float max_distance, int64_t stats[4])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_volume(s, normals3, v, k, max_distance)) return r;
    Staged st;
    const float* nd = st.in(normals3, (size_t)s->n * 3);   // (the caller's array is not retained)
    st.run([&] { return to_volume(s, nd, nullptr, v, k, max_distance, stats); });
    return st.finish("sdfk_points_to_volume");
}

extern "C" int sdfk_points_to_volume_colors_device(const sdfk_points* s, const void* normals3_dev, const void* colors3_dev, sdfk_volume* v, int32_t k,
                                                   float max_distance, int64_t stats[4])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_volume_colors(s, normals3_dev, colors3_dev, v, k, max_distance)) return r;
    return to_volume(s, (const float*)normals3_dev, (const float*)colors3_dev, v, k, max_distance, stats);
}

extern "C" int sdfk_points_to_volume_colors(const sdfk_points* s, const float* normals3, const float* colors3, sdfk_volume* v, int32_t k,
                                            float max_distance, int64_t stats[4])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_volume_colors(s, normals3, colors3, v, k, max_distance)) return r;
    Staged st;
    const float* nd = st.in(normals3, (size_t)s->n * 3);   // (the caller's arrays are not retained)
    const float* cd = st.in(colors3, (size_t)s->n * 3);
    st.run([&] { return to_volume(s, nd, cd, v, k, max_distance, stats); });
    return st.finish("sdfk_points_to_volume_colors");
}

extern "C" int sdfk_points_blend_colors_device(const sdfk_points* s, const void* colors3_dev, const void* queries3_dev, int64_t n, int32_t k,
                                               float max_distance, void* colors_out_dev, void* found_dev)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_colors(s, colors3_dev, queries3_dev, n, k, max_distance)) return r;
    if (n == 0) return SDFK_OK;
    return colors_launch(s, ColorArgs{(const float*)colors3_dev, (const float*)queries3_dev, n, k, radius_d2_bound(max_distance), (float*)colors_out_dev,
                                      (int32_t*)found_dev, nullptr});
}

extern "C" int sdfk_points_blend_colors(const sdfk_points* s, const float* colors3, const float* queries3, int64_t n, int32_t k, float max_distance,
                                        float* colors_out, int32_t* found)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = check_colors(s, colors3, queries3, n, k, max_distance)) return r;
    if (n == 0) return SDFK_OK;
    Staged st;
    const float* cd = st.in(colors3, (size_t)s->n * 3);
    const float* qd = st.in(queries3, (size_t)n * 3);
    const ColorArgs A{cd, qd, n, k, radius_d2_bound(max_distance), st.out(colors_out, (size_t)n * 3), st.out(found, (size_t)n), nullptr};
    st.run([&] { return colors_launch(s, A); });
    return st.finish("sdfk_points_blend_colors");
}
