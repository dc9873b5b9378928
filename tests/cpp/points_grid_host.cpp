// points_grid_host.cpp -- the grid arithmetic of the KdTree search (sdfkit_amd/csrc/points_grid.h, compiled here as plain C++,
// the same functions the kernels call) on the boxes that stress it: every cell index of every coordinate -- the box's ends,
// values just outside, NaN, infinities -- lies in [0, dim), every key in [0, cells), the cell counts stay within their bounds,
// and cells are monotone along each axis.  Prints "grid ok" and exits 0, or the first failure and exits 1.
//
//   points_grid_host cells IN OUT   the grid and the cells of given coordinates, for tests/test_points_walk_model.py to compare
//                                   the numpy restatement (tests/meshsdf_cases.py grid_for_box / cell_of) with, bit for bit.
//                                   IN: f32 lo[3], hi[3]; i64 n, m; m x 3 f32 coordinates (any value).
//                                   OUT: i32 dim[3]; f32 h, inv_h, slack; m x 3 i32 cells (cell_of per axis).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../sdfkit_amd/csrc/points_grid.h"

using namespace sdfk_points_grid;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 10) { printf("FAIL %s:%d: %s  ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_box(const char* what, float lo[3], float hi[3], int64_t n)
{
    const Grid G = grid_for_box(lo, hi, n);
    const int64_t cells = (int64_t)G.dim[0] * G.dim[1] * G.dim[2];
    CHECK(cells >= 1 && cells <= kMaxCells, "%s: cells %lld", what, (long long)cells);
    for (int a = 0; a < 3; a++) {
        CHECK(G.dim[a] >= 1 && G.dim[a] <= kMaxAxisCells, "%s: dim[%d] = %d", what, a, G.dim[a]);
        CHECK(G.h > 0 && std::isfinite(G.h) && G.inv_h > 0 && std::isfinite(G.inv_h), "%s: h %g inv_h %g", what, G.h, G.inv_h);
        // the coordinates to try along this axis: the ends, their float neighbours, a sweep, non-finite values
        std::vector<float> xs = {lo[a], hi[a], std::nextafter(lo[a], -INFINITY), std::nextafter(hi[a], INFINITY),
                                 std::nextafter(hi[a], -INFINITY), -INFINITY, INFINITY, NAN, -std::numeric_limits<float>::max(),
                                 std::numeric_limits<float>::max()};
        for (int k = 0; k <= 4096; k++) xs.push_back(lo[a] + (float)((double)(hi[a] - lo[a]) * k / 4096.0));
        for (float x : xs) {
            const int c = cell_of(x, G.lo[a], G.inv_h, G.dim[a]);
            CHECK(c >= 0 && c < G.dim[a], "%s: axis %d x = %.9g -> cell %d of %d", what, a, x, c, G.dim[a]);
        }
        int prev = -1;
        for (int k = 0; k <= 4096; k++) {
            const int c = cell_of(xs[10 + k], G.lo[a], G.inv_h, G.dim[a]);
            CHECK(c >= prev, "%s: axis %d not monotone at %d", what, a, k);
            prev = c;
        }
    }
    int cx, cy, cz;
    const uint32_t kh = key_of(G, hi[0], hi[1], hi[2], &cx, &cy, &cz), kl = key_of(G, lo[0], lo[1], lo[2], &cx, &cy, &cz);
    CHECK((int64_t)kh < cells && kl == 0, "%s: key of hi %u, of lo %u, cells %lld", what, kh, kl, (long long)cells);
    printf("%-34s n = %-11lld dim = %d x %d x %d\n", what, (long long)n, G.dim[0], G.dim[1], G.dim[2]);
}

static int cells_mode(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    if (!f) { printf("cannot read %s\n", in_path); return 1; }
    float box[6];
    int64_t nm[2];
    if (fread(box, sizeof(float), 6, f) != 6 || fread(nm, sizeof(int64_t), 2, f) != 2 || nm[1] < 0) { printf("short input\n"); fclose(f); return 1; }
    std::vector<float> x((size_t)nm[1] * 3);
    if (fread(x.data(), sizeof(float), x.size(), f) != x.size()) { printf("short input\n"); fclose(f); return 1; }
    fclose(f);
    const Grid G = grid_for_box(box, box + 3, nm[0]);
    std::vector<int32_t> cells(x.size());
    for (size_t i = 0; i < x.size(); i++) cells[i] = cell_of(x[i], G.lo[i % 3], G.inv_h, G.dim[i % 3]);
    f = fopen(out_path, "wb");
    if (!f) { printf("cannot write %s\n", out_path); return 1; }
    const int32_t dim[3] = {G.dim[0], G.dim[1], G.dim[2]};
    const float hs[3] = {G.h, G.inv_h, G.slack};
    fwrite(dim, sizeof(int32_t), 3, f);
    fwrite(hs, sizeof(float), 3, f);
    fwrite(cells.data(), sizeof(int32_t), cells.size(), f);
    fclose(f);
    printf("cells ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "cells")) return cells_mode(argv[2], argv[3]);
    {   // a line of 20 000 000 points on x in [0, 1]: the single-axis request exceeds 2^24 cells
        float lo[3] = {0, 0, 0}, hi[3] = {1, 0, 0};
        check_box("line x [0,1], 2e7 points", lo, hi, 20000000);
        check_box("line x [0,1], 2^31 - 1 points", lo, hi, (int64_t(1) << 31) - 1);
        float lo2[3] = {0, -3, 0}, hi2[3] = {0, 5e6f, 0};
        check_box("line y [-3,5e6], 3e7 points", lo2, hi2, 30000000);
    }
    {   // a thin plane and a long thin box
        float lo[3] = {0, 0, 0}, hi[3] = {1, 1e-7f, 1};
        check_box("near-plane, 1e8 points", lo, hi, 100000000);
        float lo2[3] = {-1e6f, 0, 0}, hi2[3] = {1e6f, 1e-3f, 1e-3f};
        check_box("needle, 5e7 points", lo2, hi2, 50000000);
    }
    {   // extremes: the whole float range, one point, all points equal, tiny boxes
        const float M = std::numeric_limits<float>::max();
        float lo[3] = {-M, -M, -M}, hi[3] = {M, M, M};
        check_box("whole float range, 1e6 points", lo, hi, 1000000);
        float p[3] = {0.25f, -1, 3};
        check_box("all equal, 1000 points", p, p, 1000);
        check_box("one point", p, p, 1);
        float lo2[3] = {1, 1, 1}, hi2[3] = {std::nextafter(1.0f, 2.0f), 1, 1};
        check_box("two adjacent floats, 2e7 points", lo2, hi2, 20000000);
    }
    {   // random boxes and counts
        std::mt19937_64 rng(7);
        std::uniform_real_distribution<float> u(-1000, 1000);
        std::uniform_int_distribution<int> e(-8, 8);
        for (int t = 0; t < 200; t++) {
            float lo[3], hi[3];
            for (int a = 0; a < 3; a++) {
                lo[a] = u(rng);
                hi[a] = lo[a] + (t % 3 == a ? 0.0f : std::ldexp(1.0f, e(rng)) * std::fabs(u(rng)) / 1000.0f);
            }
            const int64_t n = int64_t(1) << (t % 31);
            char what[64];
            snprintf(what, sizeof what, "random box %d", t);
            if (t % 50 == 0) check_box(what, lo, hi, n);
            else {   // (quiet)
                const Grid G = grid_for_box(lo, hi, n);
                for (int a = 0; a < 3; a++) {
                    CHECK(G.dim[a] >= 1 && G.dim[a] <= kMaxAxisCells, "random %d dim[%d] = %d", t, a, G.dim[a]);
                    CHECK(cell_of(hi[a], G.lo[a], G.inv_h, G.dim[a]) < G.dim[a], "random %d axis %d", t, a);
                }
                CHECK((int64_t)G.dim[0] * G.dim[1] * G.dim[2] <= kMaxCells, "random %d cells", t);
            }
        }
    }
    if (g_fail) { printf("%d failures\n", g_fail); return 1; }
    printf("grid ok\n");
    return 0;
}
