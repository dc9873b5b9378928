// voxelsdf_suite.cpp -- voxel volumes inside SDF programs through the C++ host layer include/SdfKit.hpp (Voxels::operator[](Vec3),
// SampleAt, SampleColor, ToSdf): the reference's indexer at arbitrary points, interpolation at the cell centres, the version counter,
// and a union with a box meshed with and without the stored volume.  Runs on the GPU (tests/test_gpu_voxel_sdf_cpp.py builds it).
#include <cmath>
#include <cstdio>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define IS_TRUE(c) do { if (!(c)) { printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)
#define TEST(name) static void name(); static void run_##name() { g_run++; printf("%s\n", #name); name(); } static void name()

static void Fill(Voxels& v)
{
    for (int x = 0; x < v.NX; x++)
        for (int y = 0; y < v.NY; y++)
            for (int z = 0; z < v.NZ; z++) v(x, y, z) = std::sin(0.7f * x) + 0.3f * y - 0.11f * z * z;
}

TEST(IndexerIsTheReferenceIndexer)
{
    Voxels v(Vector3(-1.0f, -0.5f, -2.0f), Vector3(1.5f, 1.0f, 1.0f), 11, 7, 13);
    Fill(v);
    Sdf s = Sdfs::Solid([&v](Vec3 p) { return v[p]; });
    std::vector<Vector3> pts;
    for (int i = 0; i < 4000; i++) {
        const float t = (float)i;
        pts.push_back(Vector3(-1.2f + std::fmod(t * 0.3713f, 2.9f), -0.7f + std::fmod(t * 0.1931f, 1.9f), -2.2f + std::fmod(t * 0.7717f, 3.4f)));
    }
    std::vector<Vector4> out;
    s.Sample(pts, out);
    int checked = 0;
    for (size_t i = 0; i < pts.size(); i++) {
        const Vector3 p = pts[i];
        const float qx = (p.X - v.Min.X) / v.DX, qy = (p.Y - v.Min.Y) / v.DY, qz = (p.Z - v.Min.Z) / v.DZ;
        const int ix = (int)qx, iy = (int)qy, iz = (int)qz;   // Voxels.cs:48-56 (C# (int) truncates)
        if (qx <= -1 || qy <= -1 || qz <= -1 || ix >= v.NX || iy >= v.NY || iz >= v.NZ) continue;   // the reference throws there
        checked++;
        IS_TRUE(out[i].W == v(ix, iy, iz));
        IS_TRUE(out[i].X == 1.0f && out[i].Y == 1.0f && out[i].Z == 1.0f);
    }
    IS_TRUE(checked > 2000);
}

TEST(InterpolationAtTheCellCentres)
{
    Voxels v(Vector3(-1.0f), Vector3(1.0f), 16, 12, 10);
    Fill(v);
    Voxels w = Voxels::SampleSdf(v.ToSdf(true), Vector3(-1.0f), Vector3(1.0f), 16, 12, 10);
    double worst = 0;
    for (int x = 0; x < 16; x++)
        for (int y = 0; y < 12; y++)
            for (int z = 0; z < 10; z++) worst = std::fmax(worst, std::fabs(w(x, y, z) - v(x, y, z)));
    IS_TRUE(worst <= 1e-5);
}

TEST(EditsReachTheSdf)
{
    Voxels v(Vector3(-1.0f), Vector3(1.0f), 8, 8, 8);
    Fill(v);
    Sdf s = v.ToSdf(false);
    std::vector<Vector3> pts = {Vector3(0.1f, 0.1f, 0.1f)};
    std::vector<Vector4> out;
    s.Sample(pts, out);
    IS_TRUE(out[0].W == v(4, 4, 4));
    v(4, 4, 4) = 42.0f;
    s.Sample(pts, out);
    IS_TRUE(out[0].W == 42.0f);
}

TEST(UnionWithABoxElidedIsStored)
{
    Voxels v(Vector3(-1.25f), Vector3(1.25f), 40, 40, 40);
    v.SampleSdf(Sdfs::Sphere(1.0f));
    Sdf s([&v](Vec3 p) { return Vec4(Vec3(Vector3(1.0f)), MathF::Min(v.SampleAt(p), BoxDistance(p - Vec3(Vector3(0.8f, 0.0f, 0.0f)), Vector3(0.3f)))); }, true);
    SetOption(SDFK_OPT_ELIDE_VOLUME, 0);
    Mesh a = s.ToMesh(Vector3(-1.5f), Vector3(1.5f), 264, 260, 256);
    SetOption(SDFK_OPT_ELIDE_VOLUME, 2);
    Mesh b = s.ToMesh(Vector3(-1.5f), Vector3(1.5f), 264, 260, 256);
    IS_TRUE(a.Vertices.size() > 1000);
    IS_TRUE(a.Triangles == b.Triangles);
    bool same = a.Vertices.size() == b.Vertices.size();
    for (size_t i = 0; same && i < a.Vertices.size(); i++)
        same = a.Vertices[i].X == b.Vertices[i].X && a.Vertices[i].Y == b.Vertices[i].Y && a.Vertices[i].Z == b.Vertices[i].Z;
    IS_TRUE(same);
}

int main()
{
    run_IndexerIsTheReferenceIndexer(); run_InterpolationAtTheCellCentres(); run_EditsReachTheSdf(); run_UnionWithABoxElidedIsStored();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
