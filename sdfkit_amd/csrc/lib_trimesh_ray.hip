// lib_trimesh_ray.hip -- rays against triangle meshes: sdfk_trimesh_raycast (the first hit, or any hit, of every ray) and
// sdfk_trimesh_render (one camera ray per pixel, depth / Lambert colour / triangle images).  Contract: include/sdfkit_hip.h,
// "Triangle meshes: ray casting".  Arithmetic and the grid walk: trimesh_ray.h (shared with a host test, which runs the same walk).
//
// The handle (trimesh_handle.h) is only read: the packed triangles, `list` and the x-fastest `starts` of the grid that
// sdfk_trimesh_create binned them into.  One lane per ray, 256-lane blocks, the whole per-ray state in registers; the walk goes slab
// by slab along the ray's dominant axis and hands each x run of cells to the caster as one range of `list`.  The render kernel makes
// its ray as the ray marcher does (row-major pixels: neighbouring lanes walk nearly the same cells), calls the same walk, and shades.
// Host side: trimesh_check, a Staged for the host forms' device copies, the library stream; nothing is kept on the handle but the
// two diagnostic counts of a profiled call.
#include "lib_internal.h"
#include "device_wave.h"
#include "trimesh_handle.h"
#include "trimesh_ray.h"

namespace {

using namespace sdfk_trimesh_ray;

constexpr int kBlock = 256;

struct RayGrid {
    const TriPack* tri;
    const uint32_t* list;
    const uint32_t* starts;
    Grid G;
};

struct RayOut {
    int32_t* triangle;
    float* distance;
    float* weights3;
    unsigned long long* tests;
};

template <bool ANY>
__global__ __launch_bounds__(kBlock) void k_tm_raycast(RayGrid S, const float* __restrict__ origins, const float* __restrict__ directions,
                                                       int64_t n, double tmin, double tmax, RayOut O)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool active = i < n;
    float o[3] = {NAN, NAN, NAN}, d[3] = {NAN, NAN, NAN};
    if (active)
        for (int a = 0; a < 3; a++) { o[a] = origins[3 * i + a]; d[a] = directions[3 * i + a]; }
    const Ray R = ray_setup(o, d, tmin, tmax);
    const PackTris T{S.tri};
    Caster<PackTris, ANY> C(T, S.list, R);
    walk(S.G, S.starts, R, C);
    wave_add(O.tests, C.tests);
    if (!active) return;
    if (O.triangle) O.triangle[i] = C.best.tri;
    if (ANY) return;
    float dist = INFINITY, w[3] = {NAN, NAN, NAN};
    if (C.best.tri >= 0) hit_outputs(C.best, &dist, w);
    if (O.distance) O.distance[i] = dist;
    if (O.weights3)
        for (int a = 0; a < 3; a++) O.weights3[3 * i + a] = w[a];
}

struct RenderArgs {
    float cam[3];
    float m[16];
    int width, height;
    float nearp, farp;
    const int32_t* idx;
    const float* colors;   // null: the mesh has none
    float* depth;
    float* rgb;
    int32_t* triangle;
    unsigned long long* tests;
};

// (four waves per SIMD: unbounded the kernel took 130 VGPRs, two over the 128 that four waves allow, and ran 8 % slower)
__global__ __launch_bounds__(kBlock, 4) void k_tm_render(RayGrid S, RenderArgs A)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool active = k < (int64_t)A.width * A.height;
    float r[3] = {NAN, NAN, NAN};
    if (active) {
        const int j = (int)(k / A.width), i = (int)(k - (int64_t)j * A.width);
        camera_ray(A.cam, A.m, A.width, A.height, i, j, r);
    }
    const Ray R = ray_setup(A.cam, r, (double)A.nearp, (double)A.farp);
    const PackTris T{S.tri};
    Caster<PackTris, false> C(T, S.list, R);
    walk(S.G, S.starts, R, C);
    wave_add(A.tests, C.tests);
    if (!active) return;
    const bool hit = C.best.tri >= 0;
    float dist = INFINITY, w[3] = {NAN, NAN, NAN};
    if (hit) hit_outputs(C.best, &dist, w);
    if (A.depth) A.depth[k] = dist;
    if (A.triangle) A.triangle[k] = C.best.tri;
    if (!A.rgb) return;
    float rgb[3] = {0.5f, 0.75f, 1.0f};
    if (hit) {
        float a[3], b[3], c[3];
        T.corners((uint32_t)C.best.tri, a, b, c);
        const float *ca = nullptr, *cb = nullptr, *cc = nullptr;
        if (A.colors) {
            const int32_t* v = A.idx + 3 * (int64_t)C.best.tri;
            ca = A.colors + 3 * (int64_t)v[0];
            cb = A.colors + 3 * (int64_t)v[1];
            cc = A.colors + 3 * (int64_t)v[2];
        }
        shade(A.cam, r, dist, w, a, b, c, ca, cb, cc, rgb);
    }
    for (int q = 0; q < 3; q++) A.rgb[3 * k + q] = rgb[q];
}

RayGrid ray_grid(const sdfk_trimesh* t) { return RayGrid{t->tri, t->list, t->starts, t->G}; }

int raycast_check(const sdfk_trimesh* t, const void* origins, const void* directions, int64_t n, float t_min, float t_max, int32_t flags,
                  const void* distance, const void* weights3, const char* who)
{
    if (int r = trimesh_check(t, who, 0)) return r;
    if (n < 0) return fail(SDFK_ERR_INVALID, "%s: n must be >= 0", who);
    if (n >= (int64_t(1) << 32)) return fail(SDFK_ERR_INVALID, "%s: 2^32 rays or more", who);
    if (t_min != t_min || t_max != t_max) return fail(SDFK_ERR_INVALID, "%s: t_min / t_max is NaN", who);
    if (t_min > t_max) return fail(SDFK_ERR_INVALID, "%s: t_min must be <= t_max", who);
    if (flags & ~SDFK_RAY_ANY_HIT) return fail(SDFK_ERR_INVALID, "%s: unknown flag bits", who);
    if ((flags & SDFK_RAY_ANY_HIT) && (distance || weights3))
        return fail(SDFK_ERR_INVALID, "%s: SDFK_RAY_ANY_HIT gives no distance and no weights: both must be NULL", who);
    if (n > 0 && (!origins || !directions)) return fail(SDFK_ERR_INVALID, "%s: null origins / directions", who);
    return SDFK_OK;
}

int raycast_launch(const sdfk_trimesh* t, const float* o, const float* d, int64_t n, float t_min, float t_max, int32_t flags, RayOut O,
                   const char* who)
{
    Staged st;
    ProfCount<1> pc;
    pc.begin(st);
    O.tests = pc.dev;
    st.run([&] {
        ProfScope ps("k_tm_raycast");
        if (flags & SDFK_RAY_ANY_HIT)
            hipLaunchKernelGGL(k_tm_raycast<true>, dim3(grid1(n)), dim3(kBlock), 0, g.stream, ray_grid(t), o, d, n, (double)t_min, (double)t_max, O);
        else
            hipLaunchKernelGGL(k_tm_raycast<false>, dim3(grid1(n)), dim3(kBlock), 0, g.stream, ray_grid(t), o, d, n, (double)t_min, (double)t_max, O);
    });
    trimesh_keep_count(st, pc, t, n);
    return st.finish(who, false);
}

int render_check(const sdfk_trimesh* t, int32_t width, int32_t height, const float* cam, const float* m, float nearp, float farp, const void* depth,
                 const void* rgb, const void* triangle, const char* who)
{
    if (int r = trimesh_check(t, who, 0)) return r;
    if (width < 1 || height < 1) return fail(SDFK_ERR_INVALID, "%s: width and height must be >= 1", who);
    if ((int64_t)width * height >= (int64_t(1) << 31)) return fail(SDFK_ERR_INVALID, "%s: 2^31 pixels or more", who);
    if (!cam || !m) return fail(SDFK_ERR_INVALID, "%s: null camera_position / view_projection_inverse", who);
    if (nearp != nearp || farp != farp) return fail(SDFK_ERR_INVALID, "%s: near_plane / far_plane is NaN", who);
    if (nearp > farp) return fail(SDFK_ERR_INVALID, "%s: near_plane must be <= far_plane", who);
    if (!depth && !rgb && !triangle) return fail(SDFK_ERR_INVALID, "%s: no image asked for", who);
    return SDFK_OK;
}

int render_launch(const sdfk_trimesh* t, int32_t width, int32_t height, const float* cam, const float* m, float nearp, float farp, float* depth,
                  float* rgb, int32_t* triangle, const char* who)
{
    RenderArgs A{};
    for (int a = 0; a < 3; a++) A.cam[a] = cam[a];
    for (int a = 0; a < 16; a++) A.m[a] = m[a];
    A.width = width; A.height = height;
    A.nearp = nearp; A.farp = farp;
    A.idx = t->idx; A.colors = t->colors;
    A.depth = depth; A.rgb = rgb; A.triangle = triangle;
    const int64_t n = (int64_t)width * height;
    Staged st;
    ProfCount<1> pc;
    pc.begin(st);
    A.tests = pc.dev;
    st.run([&] {
        ProfScope ps("k_tm_render");
        hipLaunchKernelGGL(k_tm_render, dim3(grid1(n)), dim3(kBlock), 0, g.stream, ray_grid(t), A);
    });
    trimesh_keep_count(st, pc, t, n);
    return st.finish(who, false);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_trimesh_raycast_device(const sdfk_trimesh* t, const void* origins3_dev, const void* directions3_dev, int64_t n, float t_min,
                                           float t_max, int32_t flags, void* triangle_dev, void* distance_dev, void* weights3_dev)
{
    static const char* who = "sdfk_trimesh_raycast";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = raycast_check(t, origins3_dev, directions3_dev, n, t_min, t_max, flags, distance_dev, weights3_dev, who)) return r;
    if (n == 0) return SDFK_OK;
    return raycast_launch(t, (const float*)origins3_dev, (const float*)directions3_dev, n, t_min, t_max, flags,
                          RayOut{(int32_t*)triangle_dev, (float*)distance_dev, (float*)weights3_dev, nullptr}, who);
}

extern "C" int sdfk_trimesh_raycast(const sdfk_trimesh* t, const float* origins3, const float* directions3, int64_t n, float t_min, float t_max,
                                    int32_t flags, int32_t* triangle, float* distance, float* weights3)
{
    static const char* who = "sdfk_trimesh_raycast";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = raycast_check(t, origins3, directions3, n, t_min, t_max, flags, distance, weights3, who)) return r;
    if (n == 0) return SDFK_OK;
    Staged st;
    const float* od = st.in(origins3, (size_t)n * 3);
    const float* dd = st.in(directions3, (size_t)n * 3);
    const RayOut O{st.out(triangle, (size_t)n), st.out(distance, (size_t)n), st.out(weights3, (size_t)n * 3), nullptr};
    st.run([&] { return raycast_launch(t, od, dd, n, t_min, t_max, flags, O, who); });
    return st.finish(who);
}

extern "C" int sdfk_trimesh_render_device(const sdfk_trimesh* t, int32_t width, int32_t height, const float camera_position[3],
                                          const float view_projection_inverse[16], float near_plane, float far_plane, void* depth_dev, void* rgb_dev,
                                          void* triangle_dev)
{
    static const char* who = "sdfk_trimesh_render";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = render_check(t, width, height, camera_position, view_projection_inverse, near_plane, far_plane, depth_dev, rgb_dev, triangle_dev, who))
        return r;
    return render_launch(t, width, height, camera_position, view_projection_inverse, near_plane, far_plane, (float*)depth_dev, (float*)rgb_dev,
                         (int32_t*)triangle_dev, who);
}

extern "C" int sdfk_trimesh_render(const sdfk_trimesh* t, int32_t width, int32_t height, const float camera_position[3],
                                   const float view_projection_inverse[16], float near_plane, float far_plane, float* depth, float* rgb,
                                   int32_t* triangle)
{
    static const char* who = "sdfk_trimesh_render";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = render_check(t, width, height, camera_position, view_projection_inverse, near_plane, far_plane, depth, rgb, triangle, who)) return r;
    const size_t n = (size_t)width * height;
    Staged st;
    float* dd = st.out(depth, n);
    float* cd = st.out(rgb, n * 3);
    int32_t* td = st.out(triangle, n);
    st.run([&] { return render_launch(t, width, height, camera_position, view_projection_inverse, near_plane, far_plane, dd, cd, td, who); });
    return st.finish(who);
}
