// points_knn_suite.cpp -- SdfKit::KdTree::SearchKNearest / SearchRadius (include/SdfKit.hpp) against vectors that
// tests/test_gpu_points_knn_cpp.py writes with the numpy model (tests/points_knn_model.py): every index, every distance bit,
// every found count and offset.  Runs on the GPU through libsdfkit_hip.so.
//
// File (little endian): i64 n_static, n_queries, k, total; f32 max_distance, radius; static xyz; query xyz;
// knn index (n_queries x k i32), knn distance (f32), found (i32); offsets (n_queries + 1 i64), radius index (total i32), distance.
#include <cstdio>
#include <cstring>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define CHECK(cond)                                                                                     \
    do { if (!(cond)) { printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } } while (0)
#define TEST(name) static void name(); static void run_##name() { g_run++; printf("%s\n", #name); name(); } static void name()

struct Vectors {
    int64_t ns = 0, nq = 0, k = 0, total = 0;
    float max_distance = 0, radius = 0;
    std::vector<Vector3> P, Q;
    std::vector<int32_t> knn_index, found, rad_index;
    std::vector<float> knn_distance, rad_distance;
    std::vector<int64_t> offsets;
};
static Vectors V;

template <class T>
static void read_vec(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { printf("short vector file\n"); exit(2); }
}

static void load(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    int64_t h[4];
    float r[2];
    if (fread(h, sizeof h, 1, f) != 1 || fread(r, sizeof r, 1, f) != 1) { printf("short vector file\n"); exit(2); }
    V.ns = h[0]; V.nq = h[1]; V.k = h[2]; V.total = h[3];
    V.max_distance = r[0]; V.radius = r[1];
    read_vec(f, V.P, (size_t)V.ns);
    read_vec(f, V.Q, (size_t)V.nq);
    read_vec(f, V.knn_index, (size_t)(V.nq * V.k));
    read_vec(f, V.knn_distance, (size_t)(V.nq * V.k));
    read_vec(f, V.found, (size_t)V.nq);
    read_vec(f, V.offsets, (size_t)V.nq + 1);
    read_vec(f, V.rad_index, (size_t)V.total);
    read_vec(f, V.rad_distance, (size_t)V.total);
    fclose(f);
}

template <class T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

TEST(KNearestEqualsTheModel)
{
    KdTree tree(V.P);
    const KdTree::KNearest r = tree.SearchKNearest(V.Q, (int)V.k, V.max_distance);
    CHECK(r.K == (int)V.k);
    CHECK(same_bits(r.Indices, V.knn_index));
    CHECK(same_bits(r.Distances, V.knn_distance));
    CHECK(same_bits(r.Found, V.found));
}

TEST(RadiusEqualsTheModel)
{
    KdTree tree(V.P);
    const KdTree::InRadius r = tree.SearchRadius(V.Q, V.radius);
    CHECK(same_bits(r.Offsets, V.offsets));
    CHECK(same_bits(r.Indices, V.rad_index));
    CHECK(same_bits(r.Distances, V.rad_distance));
}

TEST(OneNearestEqualsSearch)
{
    KdTree tree(V.P);
    const KdTree::KNearest r = tree.SearchKNearest(V.Q, 1);
    for (size_t i = 0; i < V.Q.size(); i++) {
        float d = 0;
        const Vector3 p = tree.Search(V.Q[i], d);
        CHECK(memcmp(&d, &r.Distances[i], 4) == 0);
        if (r.Found[i] == 0) {   // no point counts (the NaN query): -1, float.MaxValue, the first static point
            CHECK(r.Indices[i] == -1 && d == std::numeric_limits<float>::max() && p.X == V.P[0].X && p.Y == V.P[0].Y && p.Z == V.P[0].Z);
            continue;
        }
        const Vector3 s = V.P[(size_t)r.Indices[i]];
        CHECK(r.Found[i] == 1 && s.X == p.X && s.Y == p.Y && s.Z == p.Z);
        if (g_fail) break;
    }
}

TEST(ThreePointsAndRefusals)
{
    const std::vector<Vector3> three = {Vector3(0, 0, 1), Vector3(0, 1, 0), Vector3(1, 0, 0)};
    KdTree tree(three);
    const KdTree::KNearest r = tree.SearchKNearest({Vector3(0.0f, 1.5f, 0.0f)}, 8);
    CHECK(r.Found[0] == 3 && r.Indices[0] == 1 && r.Distances[0] == 0.5f);
    CHECK(r.Indices[3] == -1 && r.Distances[3] == std::numeric_limits<float>::max());
    const KdTree::InRadius a = tree.SearchRadius({Vector3(0.0f, 1.5f, 0.0f)}, 0.5f);
    CHECK(a.Offsets.size() == 2 && a.Offsets[1] == 1 && a.Indices[0] == 1 && a.Distances[0] == 0.5f);
    const KdTree::InRadius b = tree.SearchRadius({Vector3(0.0f, 1.5f, 0.0f)}, std::nextafterf(0.5f, 0.0f));
    CHECK(b.Offsets[1] == 0 && b.Indices.empty());
    int refused = 0;
    try { tree.SearchKNearest(three, 65); } catch (const std::exception&) { refused++; }
    try { tree.SearchKNearest(three, 0); } catch (const std::exception&) { refused++; }
    try { tree.SearchRadius(three, -1.0f); } catch (const std::exception&) { refused++; }
    CHECK(refused == 3);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: points_knn_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_KNearestEqualsTheModel(); run_RadiusEqualsTheModel(); run_OneNearestEqualsSearch(); run_ThreePointsAndRefusals();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
