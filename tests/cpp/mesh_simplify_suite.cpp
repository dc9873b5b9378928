// mesh_simplify_suite.cpp -- SdfKit::MeshSdf::Simplify and Mesh::Simplify (include/SdfKit.hpp) against the cases recorded from the
// numpy model in tests/golden/mesh_simplify_cases.json, which tests/test_gpu_mesh_simplify_cpp.py hands over with their meshes.
// Runs on the GPU through libsdfkit_hip.so.
//
// File (little endian): i64 cases; per case: i64 nv, nt, has_colors, runs; f32 cell, pad; vertices (nv x 3 f32), triangles
// (3 nt i32), colours (nv x 3 f32 when has_colors); then per run: i64 placement, flags, kv, kt, stats[6]; vertex_index (kv i32),
// triangle_index (kt i32), triangles (3 kt i32), vertices (kv x 3 f32), colours (kv x 3 f32).
#include <cmath>
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

struct Want {
    int64_t placement = 0, flags = 0, kv = 0, kt = 0, stats[6] = {0, 0, 0, 0, 0, 0};
    std::vector<int32_t> vi, ti, tr;
    std::vector<Vector3> V, C;
};
struct Case {
    int64_t nv = 0, nt = 0, hasColors = 0;
    float cell = 0;
    std::vector<Vector3> V, C;
    std::vector<int32_t> T;
    std::vector<Want> want;
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
    int64_t n;
    if (fread(&n, sizeof n, 1, f) != 1) { printf("short vector file\n"); exit(2); }
    Cases.resize((size_t)n);
    for (Case& c : Cases) {
        int64_t h[4];
        float t[2];
        if (fread(h, sizeof h, 1, f) != 1 || fread(t, sizeof t, 1, f) != 1) { printf("short vector file\n"); exit(2); }
        c.nv = h[0]; c.nt = h[1]; c.hasColors = h[2]; c.cell = t[0];
        c.want.resize((size_t)h[3]);
        read_into(f, c.V, (size_t)c.nv); read_into(f, c.T, (size_t)c.nt * 3);
        if (c.hasColors) read_into(f, c.C, (size_t)c.nv);
        for (Want& w : c.want) {
            int64_t k[10];
            if (fread(k, sizeof k, 1, f) != 1) { printf("short vector file\n"); exit(2); }
            w.placement = k[0]; w.flags = k[1]; w.kv = k[2]; w.kt = k[3];
            for (int i = 0; i < 6; i++) w.stats[i] = k[4 + i];
            read_into(f, w.vi, (size_t)w.kv); read_into(f, w.ti, (size_t)w.kt); read_into(f, w.tr, (size_t)w.kt * 3);
            read_into(f, w.V, (size_t)w.kv); read_into(f, w.C, (size_t)w.kv);
        }
    }
    fclose(f);
}

static bool same_bits(const std::vector<Vector3>& a, const std::vector<Vector3>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(Vector3)) == 0);
}

static const Want& find(const Case& c, int placement, int flags)
{
    for (const Want& w : c.want)
        if (w.placement == placement && w.flags == flags) return w;
    printf("no such run\n");
    exit(2);
}

TEST(RecordedCasesEqualTheModel)
{
    for (const Case& c : Cases) {
        MeshSdf m(c.V, c.T, c.C);
        for (const Want& w : c.want) {
            const MeshSimplify g = m.Simplify(c.cell, (SimplifyPlacement)w.placement, (SimplifyDuplicates)w.flags);
            CHECK(g.VertexIndex == w.vi && g.TriangleIndex == w.ti && g.Triangles == w.tr);
            CHECK(same_bits(g.Vertices, w.V) && same_bits(g.Colors, w.C));
            CHECK(g.Merged == w.stats[0] && g.DegenerateDropped == w.stats[1] && g.DuplicatesDropped == w.stats[2] && g.UnreferencedDropped == w.stats[3] &&
                  g.Passes == w.stats[4] && g.QuadricFallbacks == w.stats[5]);
            // the map sends every kept triangle's old corners to its new ones
            bool mapped = g.VertexMap.size() == (size_t)c.nv;
            for (size_t i = 0; mapped && i < g.TriangleIndex.size(); i++)
                for (int k = 0; k < 3; k++) mapped = mapped && g.VertexMap[(size_t)c.T[3 * (size_t)g.TriangleIndex[i] + k]] == g.Triangles[3 * i + k];
            CHECK(mapped);
        }
    }
}

TEST(MeshMembers)
{
    // the second case: the coloured torus
    const Case& c = Cases.at(1);
    Mesh in;
    in.Vertices = c.V; in.Triangles = c.T; in.Colors = c.C;
    for (size_t i = 0; i < c.V.size(); i++) in.Normals.push_back(Vector3(c.V[i].X, c.V[i].Y, 4.0f * c.V[i].Z));
    CHECK(in.Topology().IsWatertight());
    const Want& q = find(c, SDFK_SIMPLIFY_QUADRIC, 0);
    const Mesh m = in.Simplify(c.cell);
    CHECK(same_bits(m.Vertices, q.V) && m.Triangles == q.tr && same_bits(m.Colors, q.C) && m.Normals.size() == m.Vertices.size());
    CHECK(m.Triangles.size() < in.Triangles.size());
    const Mesh gathered = in.Simplify(c.cell, SimplifyPlacement::Quadric, SimplifyDuplicates::One, false);
    bool same = gathered.Normals.size() == q.vi.size();
    for (size_t i = 0; same && i < q.vi.size(); i++) same = memcmp(&gathered.Normals[i], &in.Normals[(size_t)q.vi[i]], sizeof(Vector3)) == 0;
    CHECK(same);
    CHECK(same_bits(m.Normals, gathered.RecomputeNormals().Normals));
    Vector3 lo = m.Vertices[0], hi = m.Vertices[0];
    for (const Vector3& v : m.Vertices) {
        lo = Vector3(std::min(lo.X, v.X), std::min(lo.Y, v.Y), std::min(lo.Z, v.Z));
        hi = Vector3(std::max(hi.X, v.X), std::max(hi.Y, v.Y), std::max(hi.Z, v.Z));
    }
    CHECK(memcmp(&m.Min, &lo, sizeof lo) == 0 && memcmp(&m.Max, &hi, sizeof hi) == 0);
    // cancelling keeps the torus watertight
    const Mesh w = in.Simplify(c.cell, SimplifyPlacement::Centroid, SimplifyDuplicates::Cancel);
    CHECK(same_bits(w.Vertices, find(c, SDFK_SIMPLIFY_CENTROID, SDFK_SIMPLIFY_CANCEL_PAIRS).V) && w.Topology().IsWatertight());
    // everything in one cell: an empty Mesh
    Mesh point;
    point.Vertices = {Vector3(1.0f, 2.0f, 3.0f), Vector3(1.5f, 2.0f, 3.0f), Vector3(1.0f, 2.5f, 3.0f)}; point.Triangles = {0, 1, 2};
    const Mesh none = point.Simplify(1.0f);
    CHECK(none.Vertices.empty() && none.Triangles.empty() && none.Normals.empty() && none.Colors.empty());
}

TEST(Refusals)
{
    const Case& c = Cases.at(0);
    MeshSdf m(c.V, c.T);
    std::vector<int32_t> out((size_t)c.nv, -7);
    int64_t kv = -7, kt = -7, st[6] = {-7, -7, -7, -7, -7, -7};
    auto call = [&](sdfk_trimesh* h, float cell, int32_t placement, int32_t flags) {
        return sdfk_trimesh_simplify(h, cell, placement, flags, out.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &kv, &kt, st);
    };
    CHECK(call(nullptr, 1.0f, 0, 0) == SDFK_ERR_INVALID);
    CHECK(call(m.Handle(), 0.0f, 0, 0) == SDFK_ERR_INVALID);
    CHECK(call(m.Handle(), -1.0f, 0, 0) == SDFK_ERR_INVALID);
    CHECK(call(m.Handle(), NAN, 0, 0) == SDFK_ERR_INVALID);
    CHECK(call(m.Handle(), INFINITY, 0, 0) == SDFK_ERR_INVALID);
    CHECK(call(m.Handle(), 1.0f, 3, 0) == SDFK_ERR_INVALID);
    CHECK(call(m.Handle(), 1.0f, -1, 0) == SDFK_ERR_INVALID);
    CHECK(call(m.Handle(), 1.0f, 0, 4) == SDFK_ERR_INVALID);
    CHECK(call(m.Handle(), 1.0f, 0, SDFK_SIMPLIFY_KEEP_DUPLICATES | SDFK_SIMPLIFY_CANCEL_PAIRS) == SDFK_ERR_INVALID);
    CHECK(std::string(sdfk_last_error()).find("sdfk_trimesh_simplify") != std::string::npos);
    CHECK(call(m.Handle(), 1e-7f, 0, 0) == SDFK_ERR_INVALID);   // 10^7 cells
    CHECK(std::string(sdfk_last_error()).find("2^21 cells") != std::string::npos);
    for (int32_t x : out) CHECK(x == -7);
    CHECK(kv == -7 && kt == -7 && st[0] == -7 && st[5] == -7);
    int refused = 0;
    try { m.Simplify(-1.0f); } catch (const std::exception&) { refused++; }
    CHECK(refused == 1);
    CHECK(m.Simplify(c.cell).VertexIndex == find(c, SDFK_SIMPLIFY_QUADRIC, 0).vi);   // (the handle is as usable as before)
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: mesh_simplify_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_RecordedCasesEqualTheModel(); run_MeshMembers(); run_Refusals();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
