// points_cluster_suite.cpp -- SdfKit::KdTree::Clusters, SelectClusters, RemoveSmallClusters and LargestCluster (include/SdfKit.hpp)
// against vectors that tests/test_gpu_points_cluster_cpp.py writes with the numpy model (tests/points_cluster_model.py): every
// output, as integers.  Runs on the GPU through libsdfkit_hip.so.
//
// File (little endian): i64 cases; per case: i64 n, C, min_points, min_size, kept, largest_kept, stats (4); f32 radius; static xyz
// (n x 3 f32); the model's labels (n i32), sizes (C i32), core (n u8), counts (n i32); the indices of the points in clusters of at
// least min_size members (kept i32) and of those in the largest cluster (largest_kept i32).
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
    int64_t n = 0, C = 0, min_points = 0, min_size = 0, kept = 0, largest_kept = 0, stats[4] = {};
    float radius = 0;
    std::vector<Vector3> P;
    std::vector<int32_t> labels, sizes, counts, indices, largest;
    std::vector<uint8_t> core;
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
        if (fread(h, sizeof h, 1, f) != 1 || fread(&c.radius, sizeof c.radius, 1, f) != 1) { printf("short vector file\n"); exit(2); }
        c.n = h[0]; c.C = h[1]; c.min_points = h[2]; c.min_size = h[3]; c.kept = h[4]; c.largest_kept = h[5];
        memcpy(c.stats, h + 6, sizeof c.stats);
        get(f, c.P, (size_t)c.n);
        get(f, c.labels, (size_t)c.n); get(f, c.sizes, (size_t)c.C); get(f, c.core, (size_t)c.n); get(f, c.counts, (size_t)c.n);
        get(f, c.indices, (size_t)c.kept); get(f, c.largest, (size_t)c.largest_kept);
    }
    fclose(f);
}

template <class T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static std::vector<Vector3> gather(const std::vector<Vector3>& P, const std::vector<int32_t>& idx)
{
    std::vector<Vector3> out;
    for (int32_t i : idx) out.push_back(P[(size_t)i]);
    return out;
}

TEST(ClustersEqualTheModel)
{
    for (const Case& c : V) {
        KdTree tree(c.P);
        KdTree::ClusterStats st;
        const KdTree::Clustered r = tree.Clusters(c.radius, (int)c.min_points, &st);
        CHECK((int64_t)r.Sizes.size() == c.C);
        CHECK(same_bits(r.Labels, c.labels) && same_bits(r.Sizes, c.sizes) && same_bits(r.Core, c.core) && same_bits(r.Counts, c.counts));
        CHECK(st.Clusters == c.stats[0] && st.Core == c.stats[1] && st.Border == c.stats[2] && st.Noise == c.stats[3]);
        CHECK(st.Rounds >= 1 && st.Rounds <= c.n + 1);
        CHECK(tree.TotalPoints() == (int)c.n);   // the tree is not changed
    }
}

TEST(SelectionsEqualTheModel)
{
    for (const Case& c : V) {
        KdTree tree(c.P);
        const KdTree::Selected r = tree.RemoveSmallClusters(c.radius, (int)c.min_points, (int)c.min_size);
        CHECK(same_bits(r.Indices, c.indices) && same_bits(r.Labels, c.labels) && same_bits(r.Points, gather(c.P, c.indices)));
        const KdTree::Selected l = tree.LargestCluster(c.radius, (int)c.min_points);
        CHECK(same_bits(l.Indices, c.largest) && same_bits(l.Points, gather(c.P, c.largest)));
        // labels that the library did not make, and no keep byte at all
        std::vector<int32_t> odd(c.labels);
        for (size_t i = 0; i < odd.size(); i++) odd[i] = (int32_t)(i % 5) - 2;
        const KdTree::Selected o = tree.SelectClusters(odd, std::vector<uint8_t>{0, 1});
        CHECK(o.Indices.size() == (size_t)((c.n + 1) / 5));   // label 1 only: i % 5 == 3
        for (int32_t i : o.Indices) CHECK(i % 5 == 3);
        CHECK(tree.SelectClusters(c.labels, std::vector<uint8_t>{}).Indices.empty());
    }
}

TEST(Refusals)
{
    const Case& c = V.at(0);
    KdTree tree(c.P);
    int refused = 0;
    try { tree.Clusters(-1.0f); } catch (const std::exception&) { refused++; }
    try { tree.Clusters(std::numeric_limits<float>::quiet_NaN()); } catch (const std::exception&) { refused++; }
    try { tree.Clusters(0.5f, 0); } catch (const std::exception&) { refused++; }
    try { tree.RemoveSmallClusters(0.5f, -2); } catch (const std::exception&) { refused++; }
    try { tree.SelectClusters(std::vector<int32_t>(3, 0), std::vector<uint8_t>{1}); } catch (const std::exception&) { refused++; }
    CHECK(refused == 5);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: points_cluster_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_ClustersEqualTheModel(); run_SelectionsEqualTheModel(); run_Refusals();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
