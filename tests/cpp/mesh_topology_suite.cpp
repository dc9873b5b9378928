// mesh_topology_suite.cpp -- SdfKit::MeshSdf::Components / Topology / Select and Mesh::SelectComponents / RemoveSmallComponents /
// LargestComponent (include/SdfKit.hpp) against the cases recorded from the numpy model in tests/golden/mesh_topology_cases.json,
// which tests/test_gpu_mesh_topology_cpp.py hands over with their meshes.  Runs on the GPU through libsdfkit_hip.so.
//
// File (little endian): i64 cases; per case: i64 nv, nt, C, kv, kt; census (8 i64); vertices (nv x 3 f32), colours (nv x 3 f32),
// triangles (3 nt i32); vertex labels (nv i32), triangle labels (nt i32), rows (8 C i64); the select case that keeps the
// even-numbered components: vertex_index (kv i32), triangle_index (kt i32), triangles (3 kt i32).
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
    int64_t nv = 0, nt = 0, C = 0, kv = 0, kt = 0, census[8] = {};
    std::vector<Vector3> V, Col;
    std::vector<int32_t> T, vertex, triangle, sel_vertex, sel_triangle, sel_triangles;
    std::vector<int64_t> rows;
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
        int64_t h[13];
        if (fread(h, sizeof h, 1, f) != 1) { printf("short vector file\n"); exit(2); }
        c.nv = h[0]; c.nt = h[1]; c.C = h[2]; c.kv = h[3]; c.kt = h[4];
        memcpy(c.census, h + 5, sizeof c.census);
        read_into(f, c.V, (size_t)c.nv); read_into(f, c.Col, (size_t)c.nv); read_into(f, c.T, (size_t)c.nt * 3);
        read_into(f, c.vertex, (size_t)c.nv); read_into(f, c.triangle, (size_t)c.nt); read_into(f, c.rows, (size_t)c.C * 8);
        read_into(f, c.sel_vertex, (size_t)c.kv); read_into(f, c.sel_triangle, (size_t)c.kt); read_into(f, c.sel_triangles, (size_t)c.kt * 3);
    }
    fclose(f);
}

static std::vector<bool> even(int64_t count)
{
    std::vector<bool> k((size_t)count);
    for (size_t i = 0; i < k.size(); i++) k[i] = i % 2 == 0;
    return k;
}

TEST(RecordedCasesEqualTheModel)
{
    for (const Case& c : Cases) {
        MeshSdf m(c.V, c.T, c.Col);
        const MeshComponents k = m.Components();
        CHECK(k.Count == c.C && k.VertexLabels == c.vertex && k.TriangleLabels == c.triangle);
        CHECK(k.Rounds >= 1 && k.Rounds <= c.nv + 1);
        const std::vector<int64_t>* cols[8] = {&k.Triangles, &k.Vertices, &k.Edges, &k.BoundaryEdges, &k.NonManifoldEdges, &k.OddEdges,
                                               &k.InconsistentEdges, &k.AreaWeights};
        for (int j = 0; j < 8; j++) {
            CHECK((int64_t)cols[j]->size() == c.C);
            for (size_t i = 0; i < (size_t)c.C && i < cols[j]->size(); i++) CHECK((*cols[j])[i] == c.rows[8 * i + j]);
        }
        for (size_t i = 0; i < (size_t)k.Count; i++) {
            CHECK(k.EulerCharacteristic(i) == c.rows[8 * i + 1] - c.rows[8 * i + 2] + c.rows[8 * i]);
            CHECK(k.IsWatertight(i) == (c.rows[8 * i + 5] == 0) && k.IsOriented(i) == (c.rows[8 * i + 6] == 0 && c.rows[8 * i + 4] == 0));
        }
        const MeshTopology t = m.Topology();
        CHECK(t.Components == c.census[0] && t.Vertices == c.census[1] && t.Edges == c.census[2] && t.BoundaryEdges == c.census[3]);
        CHECK(t.NonManifoldEdges == c.census[4] && t.OddEdges == c.census[5] && t.InconsistentEdges == c.census[6]);
        CHECK(t.DegenerateTriangles == c.census[7] && t.Triangles == c.nt - c.census[7]);
        CHECK(t.IsWatertight() == (c.census[5] == 0) && t.EulerCharacteristic() == c.census[1] - c.census[2] + t.Triangles);
        const MeshSelection s = m.Select(even(c.C));
        CHECK(s.VertexIndex == c.sel_vertex && s.TriangleIndex == c.sel_triangle && s.Triangles == c.sel_triangles);
        CHECK(s.Vertices.size() == (size_t)c.kv && s.Colors.size() == (size_t)c.kv);
        for (size_t i = 0; i < s.Vertices.size() && i < (size_t)c.kv; i++) {
            CHECK(memcmp(&s.Vertices[i], &c.V[(size_t)c.sel_vertex[i]], sizeof(Vector3)) == 0);
            CHECK(memcmp(&s.Colors[i], &c.Col[(size_t)c.sel_vertex[i]], sizeof(Vector3)) == 0);
        }
    }
}

TEST(MeshMembers)
{
    // the case with two components (tetrahedra listed out of order, an unreferenced vertex between them)
    const Case* two = nullptr;
    for (const Case& c : Cases)
        if (c.C == 2 && c.nv == 9) two = &c;
    CHECK(two != nullptr);
    if (!two) return;
    Mesh mesh;
    mesh.Vertices = two->V; mesh.Colors = two->Col; mesh.Triangles = two->T;
    mesh.Normals.resize(two->V.size());
    for (size_t i = 0; i < mesh.Normals.size(); i++) mesh.Normals[i] = Vector3((float)i, 0.5f, -1.0f);
    CHECK(mesh.Components().Count == 2 && mesh.Topology().Components == 2 && mesh.Topology().IsWatertight() && mesh.Topology().IsOriented());
    const Mesh second = mesh.SelectComponents({false, true});
    CHECK(second.Vertices.size() == 4 && second.Triangles.size() == 12 && second.Normals.size() == 4 && second.Normals[0].X == 5.0f);
    CHECK(second.Triangles[0] == 0 && second.Triangles[1] == 2 && second.Triangles[2] == 1);   // the first listed triangle, renumbered
    CHECK(second.Min.X == 3.0f && second.Max.X == 4.0f && second.Max.Y == 1.0f);
    const Mesh largest = mesh.LargestComponent();   // a full tie: the lower number
    CHECK(largest.Vertices.size() == 4 && largest.Normals[0].X == 0.0f && largest.Min.X == 0.0f);
    CHECK(mesh.RemoveSmallComponents(4).Vertices.size() == 8 && mesh.RemoveSmallComponents(5).Vertices.empty());
    CHECK(mesh.RemoveSmallComponents(0, 0.5f).Vertices.size() == 8 && mesh.RemoveSmallComponents(0, 0.51f).Triangles.empty());
    const Mesh none = mesh.SelectComponents({false, false});
    CHECK(none.Vertices.empty() && none.Triangles.empty() && none.Normals.empty());
}

TEST(Refusals)
{
    const Case& c = Cases.at(0);
    MeshSdf m(c.V, c.T);
    int refused = 0;
    try { m.Select(std::vector<bool>((size_t)c.C + 1, true)); } catch (const std::exception&) { refused++; }
    CHECK(refused == 1);
    int64_t census[8] = {-7, -7, -7, -7, -7, -7, -7, -7}, n = -7;
    CHECK(sdfk_trimesh_topology(nullptr, census, nullptr, 0) == SDFK_ERR_INVALID && census[0] == -7);
    CHECK(sdfk_trimesh_topology(m.Handle(), census, nullptr, -1) == SDFK_ERR_INVALID && census[0] == -7);
    CHECK(sdfk_trimesh_components(nullptr, nullptr, nullptr, &n, nullptr) == SDFK_ERR_INVALID && n == -7);
    CHECK(sdfk_trimesh_select(m.Handle(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n, &n) == SDFK_ERR_INVALID && n == -7);
    CHECK(sdfk_trimesh_select(nullptr, (const uint8_t*)"\1", nullptr, nullptr, nullptr, nullptr, nullptr, &n, &n) == SDFK_ERR_INVALID && n == -7);
    CHECK(m.Components().Count == c.C);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: mesh_topology_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_RecordedCasesEqualTheModel(); run_MeshMembers(); run_Refusals();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
