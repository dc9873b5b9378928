// points_color.h -- the arithmetic of per-point colours in the point-cloud pipeline (lib_pointcloud.hip: sdfk_points_blend_colors,
// sdfk_points_to_volume_colors; lib_points_filter.hip: sdfk_points_voxel_downsample_colors), written once for the device and the
// host: the blend of the neighbours' colours at a point and the mean colour of a voxel's members.  Plain C++ outside hipcc, so that
// tests/cpp/points_color_host.cpp checks it as the kernels run it; tests/pointcloud_color_model.py restates it in numpy.  Contract:
// include/sdfkit_hip.h, "Point clouds: colours".
//
// Everything here is binary64 from the f32 inputs, + - * / only, one rounding per written operation, in the order written
// (-ffp-contract=off), and one final rounding to f32 per result.  A "colour" is any three f32 per static point: nothing is clamped,
// nothing is checked for finiteness, and normals averaged through the same calls are as legitimate as RGB.
#pragma once
#include "points_filter.h"
#include "points_knn.h"

#define SDFK_COLOR_HD SDFK_KNN_HD

namespace sdfk_color {

// ---- the colour at a point -------------------------------------------------------------------------------------------------------
// The neighbours (c_j, d2_j) of the point in row order, h2 the cut-off of points_normals.h's cutoff_d2 (the d2 of neighbour k - 1
// when k were found, else the radius bound of max_distance).  Unlike the distance blend no neighbour is skipped: a point's normal
// plays no part.  When h2 > 0:  t = (double)d2_j / (double)h2,  u = 1 - t,  w = u u,  W += w,  S_c += w (double)c_jc per channel
// (three sums, each from +0.0).  colour_c = (float)(S_c / W) when W > 0, else the first neighbour's channel bit for bit (h2 == 0,
// k = 1, every d2 equal to h2).  No neighbour: (+0, +0, +0).
struct Blend {
    double S[3] = {0.0, 0.0, 0.0};
    double W = 0.0;
    float first[3] = {0.0f, 0.0f, 0.0f};
    bool any = false;
    SDFK_COLOR_HD void add(const float c[3], float d2, float h2)
    {
        if (!any) {
            first[0] = c[0]; first[1] = c[1]; first[2] = c[2];
            any = true;
        }
        if (h2 > 0.0f) {
            const double t = (double)d2 / (double)h2;
            const double u = 1.0 - t;
            const double w = u * u;
            W += w;
            S[0] += w * (double)c[0];
            S[1] += w * (double)c[1];
            S[2] += w * (double)c[2];
        }
    }
    SDFK_COLOR_HD void result(float out[3]) const
    {
        if (W > 0.0) {
            out[0] = (float)(S[0] / W); out[1] = (float)(S[1] / W); out[2] = (float)(S[2] / W);
        } else {
            out[0] = first[0]; out[1] = first[1]; out[2] = first[2];   // (+0 when nothing was found)
        }
    }
};

// ---- the mean colour of a voxel's members ------------------------------------------------------------------------------------------
// The rule of the centroid (points_filter.h): the members in ascending index are cut into chunks of kChunk; a chunk is summed in
// order from +0.0, the f32 channels widened first; the chunk sums are added in order to +0.0; mean_c = (float)(sum_c / (double)count).
using sdfk_filter::chunks_of;
using sdfk_filter::kChunk;
using sdfk_filter::Sum3;

// one chunk of `count` (<= kChunk) members; member(t): the insertion index of its t-th
template <class M>
SDFK_COLOR_HD Sum3 chunk_sum(const float* colors3, int count, M&& member)
{
    Sum3 sum;
    for (int t = 0; t < count; t++) {
        const int64_t id = member(t);
        sum.add_point(colors3[3 * id], colors3[3 * id + 1], colors3[3 * id + 2]);
    }
    return sum;
}
// a voxel of `count` members; chunk(q): the three sums of its q-th chunk
template <class C>
SDFK_COLOR_HD void group_mean(int64_t count, C&& chunk, float out[3])
{
    Sum3 total;
    const int64_t chunks = chunks_of(count);
    for (int64_t q = 0; q < chunks; q++) total.add_sum(chunk(q));
    for (int a = 0; a < 3; a++) out[a] = sdfk_filter::centroid_of(total.v[a], count);
}

}  // namespace sdfk_color
