// depth_fusion.h -- the arithmetic of sdfk_volume_integrate_depth / sdfk_depth_unproject (lib_fusion.hip): the projection of a cell
// centre into a depth image, the classification of what the pixel says about the voxel, the running weighted average, the point of
// a pixel, and the refusals of both entry points.  Contract: include/sdfkit_hip.h, "Depth images: fusion and unprojection".  f32
// throughout, every + - * / and sqrt correctly rounded in the written order.  Plain C++ outside hipcc (no contraction:
// -ffp-contract=off), so that a host program runs the very functions the kernels run (tests/cpp/depth_fusion_host.cpp) and is compared
// with the numpy model (tests/depth_fusion_model.py) bit for bit.
#pragma once
#include "trimesh_ray.h"

#include <cstdint>

#if defined(__HIPCC__)
#define SDFK_FUSE_HD __host__ __device__ __forceinline__
#else
#define SDFK_FUSE_HD inline
#endif

namespace sdfk_depth_fusion {

struct Params {
    float truncation, depth_min, depth_max, weight, max_weight;
    int carve;   // SDFK_FUSE_CARVE_BEYOND
};

struct Frame {
    float cam[3];
    float m[16];   // the forward view-projection, row-major, row vectors
    int width, height;
};

// what a pixel says about a voxel
enum Kind { SKIP = 0, SURFACE = 1, SURFACE_CLAMPED = 2, CARVED = 3 };

// Steps 1 and 2: the pixel the cell centre p projects to; false: none (behind the camera, outside the image, a NaN).  The range
// is decided in float, before the conversion: no out-of-range index is ever formed.
SDFK_FUSE_HD bool project(const Frame& F, const float p[3], int64_t* pixel)
{
    const float* m = F.m;
    const float c0 = ((p[0] * m[0] + p[1] * m[4]) + p[2] * m[8]) + m[12];
    const float c1 = ((p[0] * m[1] + p[1] * m[5]) + p[2] * m[9]) + m[13];
    const float c3 = ((p[0] * m[3] + p[1] * m[7]) + p[2] * m[11]) + m[15];
    if (!(c3 > 0.0f)) return false;
    const float wm = (float)(F.width - 1), hm = (float)(F.height - 1);
    const float u = (c0 / c3 + 1.0f) * (wm * 0.5f);
    const float v = (1.0f - c1 / c3) * (hm * 0.5f);
    const float fu = __builtin_floorf(u + 0.5f), fv = __builtin_floorf(v + 0.5f);
    if (!(fu >= 0.0f && fu <= wm && fv >= 0.0f && fv <= hm)) return false;
    *pixel = (int64_t)(int)fv * F.width + (int)fu;
    return true;
}

// Steps 3 and 4: the depth d of the voxel's pixel against the voxel's own distance from the camera -> the observation t.
SDFK_FUSE_HD Kind classify(const Frame& F, const Params& P, const float p[3], float d, float* t)
{
    const float dx = p[0] - F.cam[0], dy = p[1] - F.cam[1], dz = p[2] - F.cam[2];
    const float r = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
    if (d >= P.depth_min && d <= P.depth_max) {
        const float s = d - r;
        if (s < -P.truncation) return SKIP;
        if (s <= P.truncation) { *t = s; return SURFACE; }
        *t = P.truncation;
        return SURFACE_CLAMPED;
    }
    if (P.carve && d > P.depth_max && r <= P.depth_max) {
        *t = P.truncation;
        return CARVED;
    }
    return SKIP;
}

// Step 5: true for a first observation (a weight that is zero, negative or NaN: D never enters the arithmetic).
SDFK_FUSE_HD bool update(const Params& P, float t, float D, float W, float* D1, float* W1)
{
    if (W > 0.0f) {
        const float sum = W + P.weight;
        *D1 = (W * D + P.weight * t) / sum;
        *W1 = sum <= P.max_weight ? sum : P.max_weight;
        return false;
    }
    *D1 = t;
    *W1 = P.weight <= P.max_weight ? P.weight : P.max_weight;
    return true;
}

// the f32 cell centre of index k on an axis: first centre m = min + 0.5 d, then + k d
SDFK_FUSE_HD float centre(float m, int k, float d) { return m + (float)k * d; }

SDFK_FUSE_HD bool depth_valid(float d, float depth_min, float depth_max) { return d >= depth_min && d <= depth_max; }

// The point of pixel (i, j) at depth d: the camera ray of trimesh_ray.h, a multiply and an add per component.
SDFK_FUSE_HD void unproject(const float cam[3], const float vpi[16], int width, int height, int i, int j, float d, float point[3])
{
    float r[3];
    sdfk_trimesh_ray::camera_ray(cam, vpi, width, height, i, j, r);
    for (int a = 0; a < 3; a++) point[a] = cam[a] + r[a] * d;
}

// ---- refusals: what is wrong with the arguments, or null -------------------------------------------------------------------
struct VolumeShape {
    int nx, ny, nz, nz_global, z0;
    float gmin[3], gmax[3];
    bool storage;
};

inline bool finite_positive(float x) { return x > 0.0f && x <= FLT_MAX; }

inline const char* image_refusal(int32_t width, int32_t height)
{
    if (width < 1 || height < 1) return "width and height must be >= 1";
    if ((int64_t)width * height >= (int64_t(1) << 31)) return "2^31 pixels or more";
    return nullptr;
}

inline const char* range_refusal(float depth_min, float depth_max)
{
    if (depth_min != depth_min || depth_max != depth_max) return "depth_min / depth_max is NaN";
    if (depth_min > depth_max) return "depth_min must be <= depth_max";
    return nullptr;
}

inline const char* params_refusal(float truncation, float depth_min, float depth_max, float weight, float max_weight, int32_t flags)
{
    if (!finite_positive(truncation)) return "truncation must be finite and > 0";
    if (!finite_positive(weight)) return "weight must be finite and > 0";
    if (!(max_weight >= weight)) return "max_weight must be >= weight (+inf: no cap)";
    if (const char* e = range_refusal(depth_min, depth_max)) return e;
    if (flags & ~1) return "unknown flag bits";
    return nullptr;
}

inline const char* volumes_refusal(const VolumeShape& a, const VolumeShape& b)
{
    if (!a.storage || !b.storage) return "a volume has no storage";
    if (a.nx != b.nx || a.ny != b.ny || a.nz != b.nz) return "values and weights differ in shape";
    if (a.nz_global != b.nz_global || a.z0 != b.z0) return "values and weights are different slabs";
    for (int k = 0; k < 3; k++)
        if (a.gmin[k] != b.gmin[k] || a.gmax[k] != b.gmax[k]) return "values and weights differ in their box";
    return nullptr;
}

}  // namespace sdfk_depth_fusion
