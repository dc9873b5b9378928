// mesh_sample_suite.cpp -- SdfKit::MeshSdf::SamplePoints / Mesh::SamplePoints (include/SdfKit.hpp) against the cases recorded from
// the numpy model in tests/golden/mesh_sample_cases.json, which tests/test_gpu_mesh_sample_cpp.py hands over with their meshes:
// the first samples of every output as bits, an FNV-1a hash of all of them, and the stats.  Runs on the GPU through
// libsdfkit_hip.so.
//
// File (little endian): i64 cases; per case: i64 nv, ni, n, u64 seed, i64 stratified, stats[2], k, u64 hash; vertices (nv x 3 f32),
// colours (nv x 3 f32), triangles (ni i32); the first k points, normals, colours, weights (k x 3 f32 each) and triangles (k i32).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define CHECK(cond)                                                                                     \
    do { if (!(cond)) { printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } } while (0)
#define TEST(name) static void name(); static void run_##name() { g_run++; printf("%s\n", #name); name(); } static void name()

struct Case {
    int64_t nv = 0, ni = 0, n = 0, stratified = 0, stats[2] = {}, k = 0;
    uint64_t seed = 0, hash = 0;
    std::vector<Vector3> V, C, points, normals, colors, weights;
    std::vector<int32_t> T, triangles;
};
static std::vector<Case> Cases;

template <typename T>
static void read_into(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { printf("short vector file\n"); exit(2); }
}

static void load(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    int64_t cases = 0;
    if (fread(&cases, sizeof cases, 1, f) != 1) { printf("short vector file\n"); exit(2); }
    Cases.resize((size_t)cases);
    for (Case& c : Cases) {
        int64_t h[9];
        if (fread(h, sizeof h, 1, f) != 1) { printf("short vector file\n"); exit(2); }
        c.nv = h[0]; c.ni = h[1]; c.n = h[2]; c.seed = (uint64_t)h[3]; c.stratified = h[4]; c.stats[0] = h[5]; c.stats[1] = h[6]; c.k = h[7];
        c.hash = (uint64_t)h[8];
        read_into(f, c.V, (size_t)c.nv); read_into(f, c.C, (size_t)c.nv); read_into(f, c.T, (size_t)c.ni);
        read_into(f, c.points, (size_t)c.k); read_into(f, c.normals, (size_t)c.k); read_into(f, c.colors, (size_t)c.k);
        read_into(f, c.weights, (size_t)c.k); read_into(f, c.triangles, (size_t)c.k);
    }
    fclose(f);
}

static void fnv(uint64_t& h, const void* p, size_t bytes)
{
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 0x100000001B3ull;
}

static uint64_t hash_of(const MeshSamples& s)
{
    uint64_t h = 0xCBF29CE484222325ull;
    fnv(h, s.Points.data(), s.Points.size() * sizeof(Vector3));
    fnv(h, s.Normals.data(), s.Normals.size() * sizeof(Vector3));
    fnv(h, s.Colors.data(), s.Colors.size() * sizeof(Vector3));
    fnv(h, s.Triangles.data(), s.Triangles.size() * sizeof(int32_t));
    fnv(h, s.Weights.data(), s.Weights.size() * sizeof(Vector3));
    return h;
}

template <typename T>
static bool first_equal(const std::vector<T>& got, const std::vector<T>& want)
{
    return got.size() >= want.size() && (want.empty() || memcmp(got.data(), want.data(), want.size() * sizeof(T)) == 0);
}

TEST(RecordedCasesEqualTheModel)
{
    for (const Case& c : Cases) {
        MeshSdf m(c.V, c.T, c.C);
        const MeshSamples s = m.SamplePoints(c.n, c.seed, c.stratified != 0);
        CHECK((int64_t)s.Points.size() == c.n && (int64_t)s.Colors.size() == c.n && (int64_t)s.Triangles.size() == c.n);
        CHECK(first_equal(s.Points, c.points));
        CHECK(first_equal(s.Normals, c.normals));
        CHECK(first_equal(s.Colors, c.colors));
        CHECK(first_equal(s.Weights, c.weights));
        CHECK(first_equal(s.Triangles, c.triangles));
        CHECK(hash_of(s) == c.hash);
        CHECK(m.SampledTriangles() == c.stats[0] && m.SampleTotalWeight() == c.stats[1]);
        // the second call reads the cached prefix sums: the same bits
        CHECK(hash_of(m.SamplePoints(c.n, c.seed, c.stratified != 0)) == c.hash);
    }
}

TEST(MeshSamplePointsIsTheOneLiner)
{
    const Case& c = Cases.at(0);
    Mesh mesh;
    mesh.Vertices = c.V; mesh.Colors = c.C; mesh.Triangles = c.T;
    mesh.Normals.resize(c.V.size());
    const MeshSamples s = mesh.SamplePoints(c.n, c.seed, c.stratified != 0);
    CHECK(hash_of(s) == c.hash);
    // without colours: none come back, everything else is the same
    MeshSdf plain(c.V, c.T);
    const MeshSamples p = plain.SamplePoints(c.n, c.seed, c.stratified != 0);
    CHECK(p.Colors.empty() && first_equal(p.Points, c.points) && first_equal(p.Weights, c.weights) && first_equal(p.Triangles, c.triangles));
    // the handle still answers Search, on a sampled point with distance 0 up to the rounding of the point
    std::vector<int32_t> tri;
    std::vector<float> d;
    std::vector<Vector3> cp;
    plain.Search({p.Points[0]}, tri, d, cp);
    CHECK(tri[0] >= 0 && d[0] <= 0x1p-22f);
}

TEST(Refusals)
{
    const Case& c = Cases.at(0);
    MeshSdf m(c.V, c.T);
    int refused = 0;
    try { m.SamplePoints(-1); } catch (const std::exception&) { refused++; }
    try { m.SamplePoints(int64_t(1) << 31); } catch (const std::exception&) { refused++; }
    CHECK(refused == 2);
    CHECK(m.SamplePoints(0).Points.empty());
    // no triangle has an area
    MeshSdf flat({Vector3(0, 0, 0), Vector3(1, 1, 1), Vector3(3, 3, 3), Vector3(2, 2, 2)}, {0, 1, 2, 3, 3, 3, 0, 0, 1});
    std::string what;
    try { flat.SamplePoints(10); } catch (const std::exception& e) { what = e.what(); }
    CHECK(what.find("no triangle has an area") != std::string::npos);
    std::vector<int32_t> tri;
    std::vector<float> d;
    std::vector<Vector3> cp;
    flat.Search({Vector3(2, 2, 3)}, tri, d, cp);
    CHECK(tri[0] == 0 && d[0] > 0);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: mesh_sample_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_RecordedCasesEqualTheModel(); run_MeshSamplePointsIsTheOneLiner(); run_Refusals();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
