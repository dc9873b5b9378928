// mesh_smooth_suite.cpp -- SdfKit::MeshSdf::Adjacency / Smooth / VertexNormals and Mesh::Smooth / RecomputeNormals
// (include/SdfKit.hpp) against the cases recorded from the numpy model in tests/golden/mesh_smooth_cases.json, which
// tests/test_gpu_mesh_smooth_cpp.py hands over with their meshes.  Runs on the GPU through libsdfkit_hip.so.
//
// File (little endian): i64 cases, iterations; f32 lambda, mu; per case: i64 nv, nt, E; vertices (nv x 3 f32), triangles (3 nt
// i32); start (nv + 1 u32), neighbours (E u32), boundary (nv u8); then as f32 bits, nv x 3 each: the smoothed positions (boundary
// pinned), the normals of the mesh, the flipped normals of the smoothed positions.
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
    int64_t nv = 0, nt = 0, E = 0;
    std::vector<Vector3> V, smoothed, normals, smoothedNormalsFlipped;
    std::vector<int32_t> T;
    std::vector<uint32_t> start, nbr;
    std::vector<uint8_t> boundary;
};
static std::vector<Case> Cases;
static int64_t Iterations = 0;
static float Lambda = 0, Mu = 0;

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
    int64_t head[2];
    float factors[2];
    if (fread(head, sizeof head, 1, f) != 1 || fread(factors, sizeof factors, 1, f) != 1) { printf("short vector file\n"); exit(2); }
    Cases.resize((size_t)head[0]);
    Iterations = head[1]; Lambda = factors[0]; Mu = factors[1];
    for (Case& c : Cases) {
        int64_t h[3];
        if (fread(h, sizeof h, 1, f) != 1) { printf("short vector file\n"); exit(2); }
        c.nv = h[0]; c.nt = h[1]; c.E = h[2];
        read_into(f, c.V, (size_t)c.nv); read_into(f, c.T, (size_t)c.nt * 3);
        read_into(f, c.start, (size_t)c.nv + 1); read_into(f, c.nbr, (size_t)c.E); read_into(f, c.boundary, (size_t)c.nv);
        read_into(f, c.smoothed, (size_t)c.nv); read_into(f, c.normals, (size_t)c.nv); read_into(f, c.smoothedNormalsFlipped, (size_t)c.nv);
    }
    fclose(f);
}

static bool same_bits(const std::vector<Vector3>& a, const std::vector<Vector3>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(Vector3)) == 0);
}

TEST(RecordedCasesEqualTheModel)
{
    for (const Case& c : Cases) {
        MeshSdf m(c.V, c.T);
        const MeshAdjacency a = m.Adjacency();
        CHECK(a.Start == c.start && a.Neighbors == c.nbr && a.Boundary == c.boundary);
        for (size_t v = 0; v < (size_t)c.nv; v++) CHECK(a.Degree(v) == (int64_t)c.start[v + 1] - (int64_t)c.start[v]);
        const std::vector<Vector3> s = m.Smooth((int)Iterations, Lambda, Mu, true);
        CHECK(same_bits(s, c.smoothed));
        CHECK(same_bits(m.Smooth(0), c.V));
        CHECK(same_bits(m.VertexNormals(), c.normals));
        CHECK(same_bits(m.VertexNormals(s, true), c.smoothedNormalsFlipped));
    }
}

TEST(MeshMembers)
{
    // the closed, outward-wound tetrahedron: the geometry's normals point away from its inside
    const Case& c = Cases.at(0);
    Mesh mesh;
    mesh.Vertices = c.V; mesh.Triangles = c.T;
    mesh.Colors.assign(c.V.size(), Vector3(0.25f, 0.5f, 0.75f));
    mesh.Normals.assign(c.V.size(), Vector3(0, 0, 0));
    const Mesh r = mesh.RecomputeNormals();            // no usable normals: not flipped
    CHECK(same_bits(r.Normals, c.normals) && same_bits(r.Vertices, c.V) && r.Triangles == c.T);
    Mesh inward = r;
    for (Vector3& n : inward.Normals) n = Vector3(-n.X, -n.Y, -n.Z);
    const Mesh kept = inward.RecomputeNormals();       // the side of the present normals is kept
    CHECK(same_bits(kept.Normals, MeshSdf(mesh).VertexNormals({}, true)));
    CHECK(same_bits(inward.RecomputeNormals(false).Normals, c.normals));
    const Mesh s = r.Smooth((int)Iterations, Lambda, Mu, true, true);
    CHECK(same_bits(s.Vertices, c.smoothed) && s.Triangles == c.T && same_bits(s.Colors, mesh.Colors));
    std::vector<Vector3> unflipped = MeshSdf(mesh).VertexNormals(c.smoothed);
    CHECK(same_bits(s.Normals, unflipped));
    Vector3 lo = s.Vertices[0], hi = s.Vertices[0];
    for (const Vector3& v : s.Vertices) {
        lo = Vector3(std::min(lo.X, v.X), std::min(lo.Y, v.Y), std::min(lo.Z, v.Z));
        hi = Vector3(std::max(hi.X, v.X), std::max(hi.Y, v.Y), std::max(hi.Z, v.Z));
    }
    CHECK(memcmp(&s.Min, &lo, sizeof lo) == 0 && memcmp(&s.Max, &hi, sizeof hi) == 0);
    CHECK(same_bits(r.Smooth(2, 0.5f, 0.0f, true, false).Normals, r.Normals));
}

TEST(Refusals)
{
    const Case& c = Cases.at(0);
    MeshSdf m(c.V, c.T);
    std::vector<float> out((size_t)c.nv * 3, -7.0f);
    int64_t n = -7;
    CHECK(sdfk_trimesh_adjacency(nullptr, nullptr, nullptr, nullptr, &n) == SDFK_ERR_INVALID && n == -7);
    CHECK(sdfk_trimesh_smooth(nullptr, 1, 0.5f, 0.0f, 0, out.data()) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_smooth(m.Handle(), 1, 0.5f, 0.0f, 0, nullptr) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_smooth(m.Handle(), -1, 0.5f, 0.0f, 0, out.data()) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_smooth(m.Handle(), 65537, 0.5f, 0.0f, 0, out.data()) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_smooth(m.Handle(), 1, NAN, 0.0f, 0, out.data()) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_smooth(m.Handle(), 1, 0.5f, INFINITY, 0, out.data()) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_smooth(m.Handle(), 1, 0.5f, 0.0f, 8, out.data()) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_vertex_normals(m.Handle(), nullptr, 0, nullptr) == SDFK_ERR_INVALID);
    CHECK(sdfk_trimesh_vertex_normals(m.Handle(), nullptr, 2, out.data()) == SDFK_ERR_INVALID);
    CHECK(std::string(sdfk_last_error()).find("sdfk_trimesh_vertex_normals") != std::string::npos);
    for (float x : out) CHECK(x == -7.0f);
    int refused = 0;
    try { m.VertexNormals(std::vector<Vector3>((size_t)c.nv + 1)); } catch (const std::exception&) { refused++; }
    CHECK(refused == 1);
    CHECK(same_bits(m.VertexNormals(), c.normals));
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: mesh_smooth_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_RecordedCasesEqualTheModel(); run_MeshMembers(); run_Refusals();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
