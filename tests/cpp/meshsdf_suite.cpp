// meshsdf_suite.cpp -- triangle-mesh distance through the C++ host layer include/SdfKit.hpp (SdfKit::MeshSdf): a 12-triangle box
// against Sdfs::Box sampled on the same grid, closest-point queries, the band, and a marching-cubes sphere mesh round trip.
// Runs on the GPU through libsdfkit_hip.so (tests/test_gpu_meshsdf_cpp.py builds it).
#include <cmath>
#include <cstdio>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define IS_TRUE(c) do { if (!(c)) { printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)
#define TEST(name) static void name(); static void run_##name() { g_run++; printf("%s\n", #name); name(); } static void name()

static void BoxMesh(Vector3 lo, Vector3 hi, std::vector<Vector3>& V, std::vector<int32_t>& T)
{
    V.clear();
    for (int i = 0; i < 8; i++) V.push_back(Vector3(i & 1 ? hi.X : lo.X, i & 2 ? hi.Y : lo.Y, i & 4 ? hi.Z : lo.Z));
    T = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
}

TEST(BoxMeshMatchesSdfsBox)
{
    std::vector<Vector3> V;
    std::vector<int32_t> T;
    BoxMesh(Vector3(-0.6f, -0.45f, -0.3f), Vector3(0.6f, 0.45f, 0.3f), V, T);
    MeshSdf m(V, T);
    Voxels a = m.ToVoxels(Vector3(-1), Vector3(1), 20, 18, 16);
    Voxels b = Voxels::SampleSdf(Sdfs::Box(Vector3(0.6f, 0.45f, 0.3f)), Vector3(-1), Vector3(1), 20, 18, 16);
    const float tol = 8 * (std::nextafter(0.6f, 1.0f) - 0.6f);
    int bad = 0, inside = 0;
    for (int x = 0; x < 20; x++)
        for (int y = 0; y < 18; y++)
            for (int z = 0; z < 16; z++) {
                const float va = a(x, y, z), vb = b(x, y, z);
                if (!(std::fabs(va - vb) <= tol)) bad++;
                if (std::fabs(vb) > 2e-5f && (va < 0) != (vb < 0)) bad++;
                inside += va < 0;
            }
    IS_TRUE(bad == 0);
    IS_TRUE(inside > 0);
}

TEST(SearchClosestPoints)
{
    std::vector<Vector3> V;
    std::vector<int32_t> T;
    BoxMesh(Vector3(-1), Vector3(1), V, T);
    MeshSdf m(V, T);
    std::vector<int32_t> tri;
    std::vector<float> d;
    std::vector<Vector3> cp;
    m.Search({Vector3(0, 0, 3), Vector3(2, 2, 2), Vector3(0.5f, 0, 0), Vector3(NAN, 0, 0)}, tri, d, cp);
    IS_TRUE(d[0] == 2.0f && cp[0].Z == 1.0f && tri[0] >= 0);
    IS_TRUE(d[1] == std::sqrt(3.0f) && cp[1].X == 1.0f && cp[1].Y == 1.0f && cp[1].Z == 1.0f);
    IS_TRUE(d[2] == 0.5f && cp[2].X == 1.0f);
    IS_TRUE(tri[3] == -1);
}

TEST(BandClampsWithExactSign)
{
    std::vector<Vector3> V;
    std::vector<int32_t> T;
    BoxMesh(Vector3(-0.5f), Vector3(0.5f), V, T);
    MeshSdf m(V, T);
    Voxels a = m.ToVoxels(Vector3(-2), Vector3(2), 16, 16, 16);
    Voxels b = m.ToVoxels(Vector3(-2), Vector3(2), 16, 16, 16, 0.3f);
    int bad = 0, clamped = 0;
    for (int x = 0; x < 16; x++)
        for (int y = 0; y < 16; y++)
            for (int z = 0; z < 16; z++) {
                const float va = a(x, y, z), vb = b(x, y, z);
                if (std::fabs(va) <= 0.3f) bad += va != vb;
                else { clamped++; bad += std::fabs(vb) != 0.3f || (va < 0) != (vb < 0); }
            }
    IS_TRUE(bad == 0);
    IS_TRUE(clamped > 0);
}

TEST(MarchingCubesSphereRoundTrip)
{
    Mesh mesh = Sdfs::Sphere(1.0f).ToMesh(Vector3(-1.5f), Vector3(1.5f), 40, 40, 40);
    MeshSdf m(mesh);
    Voxels v = m.ToVoxels(Vector3(-1.5f), Vector3(1.5f), 24, 24, 24);
    // within one marching-cubes cell of the analytic distance, and of its sign beyond one cell
    int bad = 0;
    float worst = 0;
    const float h = 3.0f / 24, cell = 3.0f / 40;
    for (int x = 0; x < 24; x++)
        for (int y = 0; y < 24; y++)
            for (int z = 0; z < 24; z++) {
                const float px = -1.5f + h * (x + 0.5f), py = -1.5f + h * (y + 0.5f), pz = -1.5f + h * (z + 0.5f);
                const float ana = std::sqrt(px * px + py * py + pz * pz) - 1.0f, got = v(x, y, z);
                worst = std::max(worst, std::fabs(got - ana));
                if (std::fabs(got - ana) > cell) bad++;
                if (std::fabs(ana) > cell && (got < 0) != (ana < 0)) bad++;
            }
    printf("  %zu triangles, worst |mesh - analytic| = %g\n", mesh.Triangles.size() / 3, worst);
    IS_TRUE(bad == 0);
}

int main()
{
    run_BoxMeshMatchesSdfsBox(); run_SearchClosestPoints(); run_BandClampsWithExactSign(); run_MarchingCubesSphereRoundTrip();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
