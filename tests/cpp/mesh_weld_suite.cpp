// mesh_weld_suite.cpp -- SdfKit::MeshSdf::Weld and Mesh::Weld / Concat (include/SdfKit.hpp) against the cases recorded from the
// numpy model in tests/golden/mesh_weld_cases.json, which tests/test_gpu_mesh_weld_cpp.py hands over with their meshes.  Runs
// on the GPU through libsdfkit_hip.so.
//
// File (little endian): i64 cases; per case: i64 nv, nt, has_colors, passes; f32 tolerance, pad; vertices (nv x 3 f32), triangles
// (3 nt i32), colours (nv x 3 f32 when has_colors); then for the flags 0, 1, 2, 3: i64 kv, kt, merged, degenerate, unreferenced;
// vertex_map (nv i32), vertex_index (kv i32), triangle_index (kt i32), triangles (3 kt i32).
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
    int64_t kv = 0, kt = 0, merged = 0, degenerate = 0, unreferenced = 0;
    std::vector<int32_t> vmap, vi, ti, tr;
};
struct Case {
    int64_t nv = 0, nt = 0, hasColors = 0, passes = 0;
    float tolerance = 0;
    std::vector<Vector3> V, C;
    std::vector<int32_t> T;
    Want want[4];
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
        c.nv = h[0]; c.nt = h[1]; c.hasColors = h[2]; c.passes = h[3]; c.tolerance = t[0];
        read_into(f, c.V, (size_t)c.nv); read_into(f, c.T, (size_t)c.nt * 3);
        if (c.hasColors) read_into(f, c.C, (size_t)c.nv);
        for (Want& w : c.want) {
            int64_t k[5];
            if (fread(k, sizeof k, 1, f) != 1) { printf("short vector file\n"); exit(2); }
            w.kv = k[0]; w.kt = k[1]; w.merged = k[2]; w.degenerate = k[3]; w.unreferenced = k[4];
            read_into(f, w.vmap, (size_t)c.nv); read_into(f, w.vi, (size_t)w.kv); read_into(f, w.ti, (size_t)w.kt); read_into(f, w.tr, (size_t)w.kt * 3);
        }
    }
    fclose(f);
}

static bool same_bits(const std::vector<Vector3>& a, const std::vector<Vector3>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(Vector3)) == 0);
}

static std::vector<Vector3> gather(const std::vector<Vector3>& from, const std::vector<int32_t>& index)
{
    std::vector<Vector3> out;
    for (int32_t i : index) out.push_back(from[(size_t)i]);
    return out;
}

TEST(RecordedCasesEqualTheModel)
{
    for (const Case& c : Cases) {
        MeshSdf m(c.V, c.T, c.C);
        for (int flags = 0; flags < 4; flags++) {
            const Want& w = c.want[flags];
            const MeshWeld g = m.Weld(c.tolerance, (flags & 1) != 0, (flags & 2) != 0);
            CHECK(g.VertexMap == w.vmap && g.VertexIndex == w.vi && g.TriangleIndex == w.ti && g.Triangles == w.tr);
            CHECK(same_bits(g.Vertices, gather(c.V, w.vi)));
            CHECK(same_bits(g.Colors, c.hasColors ? gather(c.C, w.vi) : std::vector<Vector3>(w.vi.size(), Vector3(0, 0, 0))));
            CHECK(g.Merged == w.merged && g.DegenerateDropped == w.degenerate && g.UnreferencedDropped == w.unreferenced && g.Passes == c.passes);
        }
    }
}

TEST(MeshMembers)
{
    // the first case: the soup of the closed, outward-wound tetrahedron
    const Case& c = Cases.at(0);
    const Want& w = c.want[0];
    Mesh soup;
    soup.Vertices = c.V; soup.Triangles = c.T;
    soup.Colors.assign(c.V.size(), Vector3(0.25f, 0.5f, 0.75f));
    for (size_t i = 0; i < c.V.size(); i++) soup.Normals.push_back(Vector3((float)i, 1.0f, 0.0f));
    CHECK(soup.Topology().Components == c.nt && !soup.Topology().IsWatertight());
    const Mesh m = soup.Weld();
    CHECK(same_bits(m.Vertices, gather(c.V, w.vi)) && m.Triangles == w.tr && same_bits(m.Normals, gather(soup.Normals, w.vi)));
    CHECK(same_bits(m.Colors, gather(soup.Colors, w.vi)));
    const MeshTopology t = m.Topology();
    CHECK(t.Components == 1 && t.IsWatertight() && t.IsOriented() && t.EulerCharacteristic() == 2);
    Vector3 lo = m.Vertices[0], hi = m.Vertices[0];
    for (const Vector3& v : m.Vertices) {
        lo = Vector3(std::min(lo.X, v.X), std::min(lo.Y, v.Y), std::min(lo.Z, v.Z));
        hi = Vector3(std::max(hi.X, v.X), std::max(hi.Y, v.Y), std::max(hi.Z, v.Z));
    }
    CHECK(memcmp(&m.Min, &lo, sizeof lo) == 0 && memcmp(&m.Max, &hi, sizeof hi) == 0);
    // normals = true: from the welded geometry (the gathered ones decide the side; here they point outwards at three of four)
    const Mesh r = soup.Weld(0.0f, true);
    CHECK(same_bits(r.Normals, m.RecomputeNormals().Normals) && same_bits(r.Vertices, m.Vertices));
    // welding the welded mesh is the identity
    const Mesh again = m.Weld();
    CHECK(same_bits(again.Vertices, m.Vertices) && again.Triangles == m.Triangles && same_bits(again.Normals, m.Normals));
    // Concat: two copies, the second moved: 2 components after the weld; in one place: one doubled surface
    Mesh far = soup;
    for (Vector3& v : far.Vertices) v = v + Vector3(4, 0, 0);
    const Mesh both = Mesh::Concat({soup, far});
    CHECK(both.Vertices.size() == 2 * soup.Vertices.size() && both.Triangles.size() == 2 * soup.Triangles.size());
    CHECK(both.Triangles.back() == (int32_t)both.Vertices.size() - 1 && both.Max.X == 5.0f && both.Min.X == 0.0f);
    const Mesh welded = both.Weld();
    CHECK(welded.Components().Count == 2 && welded.Vertices.size() == 8);
    const Mesh twice = Mesh::Concat({m, m}).Weld();
    CHECK(twice.Vertices.size() == 4 && twice.Triangles.size() == 24 && twice.Topology().NonManifoldEdges == 6);
    CHECK(Mesh::Concat({}).Vertices.empty());
    // everything welding to nothing: an empty Mesh
    Mesh point;
    point.Vertices.assign(3, Vector3(1, 2, 3)); point.Triangles = {0, 1, 2};
    const Mesh none = point.Weld();
    CHECK(none.Vertices.empty() && none.Triangles.empty() && none.Normals.empty());
}

TEST(Refusals)
{
    const Case& c = Cases.at(0);
    MeshSdf m(c.V, c.T);
    std::vector<int32_t> out((size_t)c.nv, -7);
    int64_t kv = -7, kt = -7, st[4] = {-7, -7, -7, -7};
    CHECK(sdfk_trimesh_weld(nullptr, 0.0f, 0, out.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &kv, &kt, st) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_weld(m.Handle(), -1.0f, 0, out.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &kv, &kt, st) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_weld(m.Handle(), NAN, 0, out.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &kv, &kt, st) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_weld(m.Handle(), INFINITY, 0, out.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &kv, &kt, st) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_weld(m.Handle(), 0.0f, 4, out.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &kv, &kt, st) == SDFK_ERR_INVALID);
    CHECK(std::string(sdfk_last_error()).find("sdfk_trimesh_weld") != std::string::npos);
    CHECK(sdfk_trimesh_weld(m.Handle(), 1e-7f, 0, out.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &kv, &kt, st) == SDFK_ERR_INVALID);   // 10^7 cells
    CHECK(std::string(sdfk_last_error()).find("2^21 cells") != std::string::npos);
    for (int32_t x : out) CHECK(x == -7);
    CHECK(kv == -7 && kt == -7 && st[0] == -7 && st[3] == -7);
    int refused = 0;
    try { m.Weld(-1.0f); } catch (const std::exception&) { refused++; }
    CHECK(refused == 1);
    CHECK(m.Weld().VertexMap == c.want[0].vmap);   // (the handle is as usable as before)
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: mesh_weld_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_RecordedCasesEqualTheModel(); run_MeshMembers(); run_Refusals();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
