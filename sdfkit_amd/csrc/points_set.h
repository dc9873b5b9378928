// points_set.h -- the handle behind sdfk_points_* (KdTree): the static points and their search grid, built by lib_points.hip and
// read by every query of the family (lib_points.hip, lib_points_knn.hip, lib_pointcloud.hip, lib_orient.hip, lib_points_filter.hip) through the walk of
// points_walk.h.  What owns the device memory of one call (Staged: the scratch of a work function, what the handle adopts, the
// device copies of a host form's arrays) is in device_stage.h, included here for them.
#pragma once
#include "lib_internal.h"
#include "device_stage.h"
#include "points_grid.h"

struct sdfk_points {
    DeviceState* owner = &cur_state();
    int64_t n = 0;
    float* xyz = nullptr;          // n x 3, insertion order (the source of every rebuild)
    float4* sorted = nullptr;      // n, cell order: (x, y, z, bits(index))
    uint32_t* starts = nullptr;    // cells + 1
    int64_t cells = 0;
    sdfk_points_grid::Grid G{};
    float first[3] = {0, 0, 0};
    int64_t last_candidates = 0, last_queries = 0;   // of the last profiled query call, whichever kind
};
