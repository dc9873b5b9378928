// points_grid.h -- the uniform grid of lib_points.hip (KdTree / IterativeClosestPoint): its sizing from the point count and
// the bounding box (host) and the cell of a coordinate (host and device).  Plain C++ outside hipcc, so that the arithmetic is
// checked on the host as the kernels run it (tests/cpp/points_grid_host.cpp).
//
// Bounds: at most kMaxCells cells in all, at most kMaxAxisCells along any axis.  The per-axis bound keeps every cell index, and
// dim - 1, exact in f32 (a nearly collinear cloud of more than 2^24 points would otherwise ask for more cells along its line),
// and cell_of clamps the INTEGER index, so no coordinate -- NaN, infinite, beyond the box by rounding -- leaves [0, dim).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SDFK_GRID_HD __host__ __device__
#else
#define SDFK_GRID_HD
#endif

namespace sdfk_points_grid {

constexpr int64_t kMaxCells = int64_t(1) << 25;       // 128 MiB of cell starts
constexpr int64_t kMaxAxisCells = int64_t(1) << 24;   // every index and dim - 1 exact in f32

struct Grid {
    float lo[3], hi[3];
    float h, inv_h;
    int dim[3];
    float slack;   // absolute error bound of cell assignment / boundary positions (distance units)
};

// The cell along one axis: floor((x - lo) / h) clamped to [0, gdim - 1]; NaN -> 0.
SDFK_GRID_HD inline int cell_of(float x, float lo, float inv_h, int gdim)
{
    float t = (x - lo) * inv_h;
    t = fminf(fmaxf(t, 0.0f), (float)kMaxAxisCells);   // (2^24: exact, and not below any dim - 1)
    const int c = (int)t;
    return c < gdim - 1 ? c : gdim - 1;
}

SDFK_GRID_HD inline uint32_t key_of(const Grid& G, float x, float y, float z, int* cx, int* cy, int* cz)
{
    *cx = cell_of(x, G.lo[0], G.inv_h, G.dim[0]);
    *cy = cell_of(y, G.lo[1], G.inv_h, G.dim[1]);
    *cz = cell_of(z, G.lo[2], G.inv_h, G.dim[2]);
    return ((uint32_t)*cz * (uint32_t)G.dim[1] + (uint32_t)*cy) * (uint32_t)G.dim[0] + (uint32_t)*cx;
}

// The grid for the box [lo, hi] holding n points: the smallest cell edge h whose cell count prod(floor(extent / h) + 1) stays
// within min(n, kMaxCells) with no axis above kMaxAxisCells: about one cell per point.
inline Grid grid_for_box(const float lo[3], const float hi[3], int64_t n)
{
    Grid G{};
    double ext[3], emax = 0, amax = 0;
    for (int a = 0; a < 3; a++) {
        G.lo[a] = lo[a];
        G.hi[a] = hi[a];
        ext[a] = (double)hi[a] - (double)lo[a];
        emax = std::max(emax, ext[a]);
        amax = std::max({amax, std::fabs((double)lo[a]), std::fabs((double)hi[a])});
    }
    const double target = (double)std::min<int64_t>(std::max<int64_t>(n, 1), kMaxCells);
    auto cells_at = [&](double h) -> double {
        double c = 1;
        for (int a = 0; a < 3; a++) {
            const double ca = std::floor(ext[a] / h) + 1.0;
            if (ca > (double)kMaxAxisCells) return (double)INFINITY;
            c *= ca;
        }
        return c;
    };
    double h;
    if (emax <= 0) h = 1.0;   // every point equal: one cell
    else {
        double hi_h = emax * 1.000001, lo_h = emax / (2.0 * std::cbrt(target) + 2.0);   // cells(hi_h) = 1 <= target
        while (cells_at(lo_h) <= target) lo_h *= 0.5;
        for (int it = 0; it < 60; it++) {
            const double mid = 0.5 * (lo_h + hi_h);
            (cells_at(mid) <= target ? hi_h : lo_h) = mid;
        }
        h = hi_h;
    }
    G.h = (float)h;
    G.inv_h = (float)(1.0 / (double)G.h);
    for (int a = 0; a < 3; a++) {
        // cells along a: enough for the cell index of hi (points beyond, by rounding, are clamped into the last cell, which
        // only widens it: the search's lower bounds stay valid)
        const double c = std::floor(ext[a] / (double)G.h) + 1.0;
        G.dim[a] = (int)std::min<double>(std::max(c, 1.0), (double)kMaxAxisCells);
    }
    while ((int64_t)G.dim[0] * G.dim[1] * G.dim[2] > kMaxCells)   // (rounding of h to f32 can add a cell per axis)
        for (int a = 0; a < 3; a++) G.dim[a] = std::max(1, G.dim[a] - 1);
    G.slack = (float)((emax + amax) * 0x1p-19 + (double)G.h * 0x1p-20);
    return G;
}

}  // namespace sdfk_points_grid
