// points_filter_suite.cpp -- SdfKit::KdTree::VoxelDownsample and RemoveStatisticalOutliers (include/SdfKit.hpp) against vectors that
// tests/test_gpu_points_filter_cpp.py writes with the numpy model (tests/points_filter_model.py): every bit of every output.  Runs
// on the GPU through libsdfkit_hip.so.
//
// File (little endian): i64 cases; per case: i64 n, m, k, kept, stats (6); f32 size, origin (3), std_ratio, max_distance; static xyz
// (n x 3 f32); the model's downsample: points (m x 3 f32), counts (m i32), group (n i32); the model's outliers: points (kept x 3 f32),
// indices (kept i32), mean distance (n f32).
#include <cstdio>
#include <cstring>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define CHECK(cond)                                                                                     \
    do { if (!(cond)) { printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } } while (0)
#define TEST(name) static void name(); static void run_##name() { g_run++; printf("%s\n", #name); name(); } static void name()

struct Case {
    int64_t n = 0, m = 0, k = 0, kept = 0, stats[6] = {};
    float size = 0, origin[3] = {}, ratio = 0, maxd = 0;
    std::vector<Vector3> P, dpoints, opoints;
    std::vector<int32_t> counts, group, indices;
    std::vector<float> mean;
};
static std::vector<Case> V;

template <class T>
static void get(FILE* f, std::vector<T>& v, size_t count)
{
    v.resize(count);
    if (count && fread(v.data(), sizeof(T), count, f) != count) { printf("short vector file\n"); exit(2); }
}

static void load(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    int64_t cases = 0;
    if (fread(&cases, sizeof cases, 1, f) != 1) { printf("short vector file\n"); exit(2); }
    V.resize((size_t)cases);
    for (Case& c : V) {
        int64_t h[10];
        float g[6];
        if (fread(h, sizeof h, 1, f) != 1 || fread(g, sizeof g, 1, f) != 1) { printf("short vector file\n"); exit(2); }
        c.n = h[0]; c.m = h[1]; c.k = h[2]; c.kept = h[3];
        memcpy(c.stats, h + 4, sizeof c.stats);
        c.size = g[0]; memcpy(c.origin, g + 1, sizeof c.origin); c.ratio = g[4]; c.maxd = g[5];
        get(f, c.P, (size_t)c.n);
        get(f, c.dpoints, (size_t)c.m); get(f, c.counts, (size_t)c.m); get(f, c.group, (size_t)c.n);
        get(f, c.opoints, (size_t)c.kept); get(f, c.indices, (size_t)c.kept); get(f, c.mean, (size_t)c.n);
    }
    fclose(f);
}

template <class T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

TEST(DownsampleEqualsTheModel)
{
    for (const Case& c : V) {
        KdTree tree(c.P);
        const KdTree::Downsampled d = tree.VoxelDownsample(c.size, Vector3{c.origin[0], c.origin[1], c.origin[2]});
        CHECK((int64_t)d.Points.size() == c.m);
        CHECK(same_bits(d.Points, c.dpoints) && same_bits(d.Counts, c.counts) && same_bits(d.Group, c.group));
        // a second pass over the result changes nothing
        if (!d.Points.empty()) {
            KdTree again(d.Points);
            const KdTree::Downsampled e = again.VoxelDownsample(c.size, Vector3{c.origin[0], c.origin[1], c.origin[2]});
            CHECK(same_bits(e.Points, d.Points));
        }
    }
}

TEST(OutliersEqualTheModel)
{
    for (const Case& c : V) {
        KdTree tree(c.P);
        KdTree::OutlierStats st;
        const KdTree::Inliers r = tree.RemoveStatisticalOutliers((int)c.k, c.ratio, c.maxd, &st);
        CHECK((int64_t)r.Points.size() == c.kept);
        CHECK(same_bits(r.Points, c.opoints) && same_bits(r.Indices, c.indices) && same_bits(r.MeanDistance, c.mean));
        CHECK(st.Kept == c.stats[0] && st.Removed == c.stats[1] && st.Isolated == c.stats[2]);
        CHECK(memcmp(&st.Mu, &c.stats[3], 8) == 0 && memcmp(&st.Sigma, &c.stats[4], 8) == 0 && memcmp(&st.Threshold, &c.stats[5], 8) == 0);
        CHECK(tree.TotalPoints() == (int)c.n);   // the tree is not changed
    }
}

TEST(Refusals)
{
    const Case& c = V.at(0);
    KdTree tree(c.P);
    int refused = 0;
    try { tree.VoxelDownsample(0.0f); } catch (const std::exception&) { refused++; }
    try { tree.VoxelDownsample(-1.0f); } catch (const std::exception&) { refused++; }
    try { tree.VoxelDownsample(std::numeric_limits<float>::infinity()); } catch (const std::exception&) { refused++; }
    try { tree.VoxelDownsample(1e-30f); } catch (const std::exception&) { refused++; }   // 2^21 voxels and more
    try { tree.VoxelDownsample(1.0f, Vector3{std::numeric_limits<float>::quiet_NaN(), 0.0f, 0.0f}); } catch (const std::exception&) { refused++; }
    try { tree.RemoveStatisticalOutliers(1, 2.0f); } catch (const std::exception&) { refused++; }
    try { tree.RemoveStatisticalOutliers(65, 2.0f); } catch (const std::exception&) { refused++; }
    try { tree.RemoveStatisticalOutliers(8, -1.0f); } catch (const std::exception&) { refused++; }
    try { tree.RemoveStatisticalOutliers(8, 2.0f, -1.0f); } catch (const std::exception&) { refused++; }
    CHECK(refused == 9);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: points_filter_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_DownsampleEqualsTheModel(); run_OutliersEqualTheModel(); run_Refusals();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
