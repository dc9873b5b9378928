// lib_fusion.hip -- depth images: sdfk_volume_integrate_depth (one frame into a running weighted average of truncated signed
// distances, Curless and Levoy 1996) and sdfk_depth_unproject (a frame as a compacted point cloud).  Contract: include/sdfkit_hip.h,
// "Depth images: fusion and unprojection".  Arithmetic and refusals: depth_fusion.h (shared with a host test).
//
// k_fuse_depth is a read-modify-write stream over the two volumes with a gather from the image.  Rows of a volume are pitch() = a
// multiple of four voxels long and rows follow each other without a gap, so voxel slot 4 g .. 4 g + 3 is quad g of the whole array:
// lane g takes quad g, a wave covers 1 KiB of each volume contiguously, D and W move as aligned 16-byte loads and stores.  The lane
// projects its four cell centres first (arithmetic and a gather from the image, which stays in L2) and touches the volumes only when
// one of the four is updated: a quad outside the frustum or beyond the truncation costs no volume traffic.  The slots of a row's
// padded tail are never updated; they travel through the registers of a stored quad as the bits they were.  The four counts are
// reduced per wave, then per block, and cost one integer atomic per block and count.
// k_unproject_*: one lane per pixel, the validity flags scanned by the shared scan (device_scan.h), then a scatter.
#include "lib_internal.h"
#include "device_scan.h"
#include "device_stage.h"
#include "device_wave.h"
#include "depth_fusion.h"

namespace {

using namespace sdfk_depth_fusion;

constexpr int kBlock = 256;

struct FuseArgs {
    Frame F;
    Params P;
    float mx, my, mz, dx, dy, dz;
    int ny, nz, z0, nq;   // nq: quads per row
    int64_t nquads, npix;
    uint4* D;
    uint4* W;
    const float* depth;
    unsigned long long* stats;   // null: not counted
};

__device__ __forceinline__ float lane_of(const uint4& q, int e) { return __uint_as_float(e == 0 ? q.x : (e == 1 ? q.y : (e == 2 ? q.z : q.w))); }
__device__ __forceinline__ void set_lane(uint4& q, int e, float v)
{
    const unsigned b = __float_as_uint(v);
    if (e == 0) q.x = b; else if (e == 1) q.y = b; else if (e == 2) q.z = b; else q.w = b;
}

// the wave's sum of `n` into the block's partial sums of count `slot`
__device__ __forceinline__ void block_part(int slot, unsigned n, unsigned* s_part)
{
    n = (unsigned)wave_sum(n);   // (a block's count fits 32 bits: the low word of the sum is all that is kept)
    if ((threadIdx.x & 63) == 0) s_part[slot * 4 + (threadIdx.x >> 6)] = n;
}

__global__ __launch_bounds__(kBlock) void k_fuse_depth(FuseArgs A)
{
    __shared__ unsigned s_part[16];
    const int64_t gq = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned n_upd = 0, n_surf = 0, n_first = 0, n_pix = 0;
    if (gq < A.nquads) {
        const int64_t row = gq / A.nq;   // = i * ny + j
        const int q = (int)(gq - row * A.nq);
        const int j = (int)(row % A.ny), i = (int)(row / A.ny);
        float p[3] = {centre(A.mx, i, A.dx), centre(A.my, j, A.dy), 0.0f};
        float t[4];
        Kind kind[4];
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int k = 4 * q + e;
            kind[e] = SKIP;
            t[e] = 0.0f;
            if (k < A.nz) {   // (not the padded tail of the row)
                p[2] = centre(A.mz, A.z0 + k, A.dz);
                int64_t pixel;
                if (project(A.F, p, &pixel)) kind[e] = classify(A.F, A.P, p, A.depth[pixel], &t[e]);
            }
            any = any || kind[e] != SKIP;
        }
        if (any) {
            uint4 D = A.D[gq], W = A.W[gq];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (kind[e] == SKIP) continue;
                float D1, W1;
                const bool first = update(A.P, t[e], lane_of(D, e), lane_of(W, e), &D1, &W1);
                set_lane(D, e, D1);
                set_lane(W, e, W1);
                n_upd++;
                n_surf += kind[e] == SURFACE;
                n_first += first;
            }
            A.D[gq] = D;
            A.W[gq] = W;
        }
    }
    if (!A.stats) return;   // (uniform)
    const int64_t lanes = (int64_t)gridDim.x * kBlock;
    for (int64_t k = gq; k < A.npix; k += lanes) n_pix += depth_valid(A.depth[k], A.P.depth_min, A.P.depth_max);
    block_part(0, n_upd, s_part);
    block_part(1, n_surf, s_part);
    block_part(2, n_first, s_part);
    block_part(3, n_pix, s_part);
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned* s = s_part + 4 * threadIdx.x;
        const unsigned long long n = (unsigned long long)s[0] + s[1] + s[2] + s[3];
        if (n) atomicAdd(A.stats + threadIdx.x, n);
    }
}

struct UnprojectArgs {
    float cam[3];
    float m[16];   // the inverse view-projection
    int width, height;
    float depth_min, depth_max;
    const float* depth;
    const float* rgb;
    float* points3;
    float* colors3;
    int32_t* pixel;
};

__global__ __launch_bounds__(kBlock) void k_unproject_flags(const float* __restrict__ depth, int64_t npix, float depth_min, float depth_max,
                                                            uint32_t* __restrict__ flags)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < npix) flags[k] = depth_valid(depth[k], depth_min, depth_max) ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void k_unproject_scatter(UnprojectArgs A, const uint32_t* __restrict__ starts)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (int64_t)A.width * A.height) return;
    const uint32_t o = starts[k];
    if (starts[k + 1] == o) return;
    const int j = (int)(k / A.width), i = (int)(k - (int64_t)j * A.width);
    if (A.points3) {
        float pt[3];
        unproject(A.cam, A.m, A.width, A.height, i, j, A.depth[k], pt);
        for (int a = 0; a < 3; a++) A.points3[3 * (int64_t)o + a] = pt[a];
    }
    if (A.colors3)
        for (int a = 0; a < 3; a++) A.colors3[3 * (int64_t)o + a] = A.rgb[3 * k + a];
    if (A.pixel) A.pixel[o] = (int32_t)k;
}

VolumeShape shape_of(const sdfk_volume* v)
{
    VolumeShape s{v->nx, v->ny, v->nz, v->nz_global, v->z0, {v->gmin[0], v->gmin[1], v->gmin[2]}, {v->gmax[0], v->gmax[1], v->gmax[2]},
                  !v->elided && v->values != nullptr};
    return s;
}

int integrate_check(const sdfk_volume* values, const sdfk_volume* weights, const void* depth, int32_t width, int32_t height, const float* cam,
                    const float* m, const sdfk_fusion_params* prm, const char* who)
{
    if (int r = require_init()) return r;
    if (!values || !weights) return fail(SDFK_ERR_INVALID, "%s: null volume", who);
    if (!depth || !cam || !m || !prm) return fail(SDFK_ERR_INVALID, "%s: null depth / camera_position / view_projection / params", who);
    if (values == weights) return fail(SDFK_ERR_INVALID, "%s: values and weights are the same volume", who);
    if (values->owner != weights->owner) return fail(SDFK_ERR_INVALID, "%s: the volumes belong to different devices", who);
    if (const char* e = volumes_refusal(shape_of(values), shape_of(weights))) return fail(SDFK_ERR_INVALID, "%s: %s", who, e);
    if (const char* e = image_refusal(width, height)) return fail(SDFK_ERR_INVALID, "%s: %s", who, e);
    if (const char* e = params_refusal(prm->truncation, prm->depth_min, prm->depth_max, prm->weight, prm->max_weight, prm->flags))
        return fail(SDFK_ERR_INVALID, "%s: %s", who, e);
    return SDFK_OK;
}

int integrate_launch(sdfk_volume* values, sdfk_volume* weights, const float* depth_dev, int32_t width, int32_t height, const float* cam,
                     const float* m, const sdfk_fusion_params* prm, int64_t stats[4], const char* who)
{
    for (sdfk_volume* v : {values, weights}) {
        resolve_dependents(v);   // (a queued mesh may still read the old values)
        volume_values_changed(v);
    }
    FuseArgs A{};
    for (int a = 0; a < 3; a++) A.F.cam[a] = cam[a];
    for (int a = 0; a < 16; a++) A.F.m[a] = m[a];
    A.F.width = width; A.F.height = height;
    A.P = Params{prm->truncation, prm->depth_min, prm->depth_max, prm->weight, prm->max_weight, prm->flags & SDFK_FUSE_CARVE_BEYOND};
    float d[3], m0[3], outside;
    grid_constants(values, d, m0, &outside);
    A.mx = m0[0]; A.my = m0[1]; A.mz = m0[2];
    A.dx = d[0]; A.dy = d[1]; A.dz = d[2];
    A.ny = values->ny; A.nz = values->nz; A.z0 = values->z0;
    A.nq = values->pitch() / 4;
    A.nquads = (int64_t)values->nx * values->ny * A.nq;
    A.npix = (int64_t)width * height;
    A.D = (uint4*)values->values;
    A.W = (uint4*)weights->values;
    A.depth = depth_dev;
    Staged st;
    unsigned long long host[4] = {0, 0, 0, 0};
    ProfCount<4> pc;
    pc.begin(st, stats != nullptr);
    A.stats = pc.dev;
    st.run([&] {
        ProfScope ps("k_fuse_depth");
        hipLaunchKernelGGL(k_fuse_depth, dim3((unsigned)((A.nquads + kBlock - 1) / kBlock)), dim3(kBlock), 0, g.stream, A);
    });
    pc.end(st, host);
    if (int r = st.finish(who, false)) return r;
    if (stats)
        for (int k = 0; k < 4; k++) stats[k] = (int64_t)host[k];
    return SDFK_OK;
}

int unproject_check(const void* depth, const void* rgb, int32_t width, int32_t height, const float* cam, const float* m, float depth_min,
                    float depth_max, const void* colors3, const int64_t* n_valid, const char* who)
{
    if (int r = require_init()) return r;
    if (!depth || !cam || !m || !n_valid) return fail(SDFK_ERR_INVALID, "%s: null depth / camera_position / view_projection_inverse / n_valid", who);
    if (colors3 && !rgb) return fail(SDFK_ERR_INVALID, "%s: colors3 without rgb: it must be NULL when rgb is NULL", who);
    if (const char* e = image_refusal(width, height)) return fail(SDFK_ERR_INVALID, "%s: %s", who, e);
    if (const char* e = range_refusal(depth_min, depth_max)) return fail(SDFK_ERR_INVALID, "%s: %s", who, e);
    return SDFK_OK;
}

int unproject_launch(const float* depth, const float* rgb, int32_t width, int32_t height, const float* cam, const float* m, float depth_min,
                     float depth_max, float* points3, float* colors3, int32_t* pixel, int64_t* n_valid, const char* who)
{
    UnprojectArgs A{};
    for (int a = 0; a < 3; a++) A.cam[a] = cam[a];
    for (int a = 0; a < 16; a++) A.m[a] = m[a];
    A.width = width; A.height = height;
    A.depth_min = depth_min; A.depth_max = depth_max;
    A.depth = depth; A.rgb = rgb;
    A.points3 = points3; A.colors3 = colors3; A.pixel = pixel;
    const int64_t n = (int64_t)width * height;
    const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
    Staged st;
    uint32_t* starts = st.scratch<uint32_t>((size_t)n + 1);
    uint32_t total = 0;
    {
        ProfScope ps("k_unproject");
        st.run([&] { hipLaunchKernelGGL(k_unproject_flags, dim3(blocks), dim3(kBlock), 0, g.stream, depth, n, depth_min, depth_max, starts); });
        st.run([&] { return sdfk_scan::scan(starts, n, who); });
        if (points3 || colors3 || pixel)
            st.run([&] { hipLaunchKernelGGL(k_unproject_scatter, dim3(blocks), dim3(kBlock), 0, g.stream, A, starts); });
    }
    st.read(&total, starts + n, sizeof total);
    if (int r = st.finish(who, false)) return r;
    *n_valid = (int64_t)total;
    return SDFK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_volume_integrate_depth_device(sdfk_volume* values, sdfk_volume* weights, const void* depth_dev, int32_t width, int32_t height,
                                                  const float camera_position[3], const float view_projection[16],
                                                  const sdfk_fusion_params* prm, int64_t stats[4])
{
    static const char* who = "sdfk_volume_integrate_depth";
    StateScope in_owner_context(values ? values->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = integrate_check(values, weights, depth_dev, width, height, camera_position, view_projection, prm, who)) return r;
    return integrate_launch(values, weights, (const float*)depth_dev, width, height, camera_position, view_projection, prm, stats, who);
}

extern "C" int sdfk_volume_integrate_depth(sdfk_volume* values, sdfk_volume* weights, const float* depth, int32_t width, int32_t height,
                                           const float camera_position[3], const float view_projection[16], const sdfk_fusion_params* prm,
                                           int64_t stats[4])
{
    static const char* who = "sdfk_volume_integrate_depth";
    StateScope in_owner_context(values ? values->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = integrate_check(values, weights, depth, width, height, camera_position, view_projection, prm, who)) return r;
    Staged st;
    const float* dd = st.in(depth, (size_t)width * height);
    st.run([&] { return integrate_launch(values, weights, dd, width, height, camera_position, view_projection, prm, stats, who); });
    return st.finish(who);
}

extern "C" int sdfk_depth_unproject_device(const void* depth_dev, const void* rgb_dev, int32_t width, int32_t height, const float camera_position[3],
                                           const float view_projection_inverse[16], float depth_min, float depth_max, void* points3_dev,
                                           void* colors3_dev, void* pixel_dev, int64_t* n_valid)
{
    static const char* who = "sdfk_depth_unproject";
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = unproject_check(depth_dev, rgb_dev, width, height, camera_position, view_projection_inverse, depth_min, depth_max, colors3_dev, n_valid,
                                who))
        return r;
    return unproject_launch((const float*)depth_dev, (const float*)rgb_dev, width, height, camera_position, view_projection_inverse, depth_min,
                            depth_max, (float*)points3_dev, (float*)colors3_dev, (int32_t*)pixel_dev, n_valid, who);
}

extern "C" int sdfk_depth_unproject(const float* depth, const float* rgb, int32_t width, int32_t height, const float camera_position[3],
                                    const float view_projection_inverse[16], float depth_min, float depth_max, float* points3, float* colors3,
                                    int32_t* pixel, int64_t* n_valid)
{
    static const char* who = "sdfk_depth_unproject";
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = unproject_check(depth, rgb, width, height, camera_position, view_projection_inverse, depth_min, depth_max, colors3, n_valid, who))
        return r;
    const size_t n = (size_t)width * height;
    Staged st;
    const float* dd = st.in(depth, n);
    const float* cd = colors3 ? st.in(rgb, n * 3) : nullptr;
    float* pd = st.out(points3, n * 3);
    float* od = st.out(colors3, n * 3);
    int32_t* xd = st.out(pixel, n);
    st.run([&] { return unproject_launch(dd, cd, width, height, camera_position, view_projection_inverse, depth_min, depth_max, pd, od, xd, n_valid, who); });
    return st.finish(who);
}
