// mathops_suite.cpp -- MathF.Sin / Cos / Exp / Log / Atan2 in SDF programs through the C++ host layer include/SdfKit.hpp: the gyroid
// and the twist of tests/test_gpu_mathops.py written with SdfKit::MathF, sampled at points (SdfEx.Sample) and meshed with and without
// the stored volume.  Runs on the GPU (tests/test_gpu_mathops_cpp.py builds it and checks what it writes against the numpy model).
//   mathops_suite OUTDIR   writes OUTDIR/<scene>.ops  { int32 n, out[4]; n x sdfk_op }
//                                 OUTDIR/<scene>.pts  { n x (x, y, z) float32 }, OUTDIR/<scene>.out { n x (r, g, b, w) float32 }
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define IS_TRUE(c) do { if (!(c)) { printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static Vec4 Gyroid(Vec3 p)
{
    const Val s = 4.0f;
    const Val x = p.X * s, y = p.Y * s, z = p.Z * s;
    const Val g = (MathF::Sin(x) * MathF::Cos(y) + MathF::Sin(y) * MathF::Cos(z)) + MathF::Sin(z) * MathF::Cos(x);
    const Val w = MathF::Max(MathF::Abs(g) / 4.0f - 0.08f, p.Length() - 1.2f);
    return Vec4(0.5f + 0.5f * MathF::Sin(x), 0.5f + 0.5f * MathF::Cos(y), MathF::Exp(-p.Length()), w);
}

static Vec4 Twist(Vec3 p)
{
    const Val a = p.Y * 2.0f;
    const Val c = MathF::Cos(a), s = MathF::Sin(a);
    const Vec3 q(c * p.X - s * p.Z, p.Y, s * p.X + c * p.Z);
    return Vec4(MathF::Atan2(q.Z, q.X) / 3.1415927f, c, s, BoxDistance(q, Vector3(0.5f, 0.9f, 0.3f)));
}

static void Dump(const std::string& dir, const char* name, const Sdf& sdf)
{
    std::vector<sdfk_op> ops;
    int32_t out[4];
    sdf.Lower(ops, out);
    std::vector<Vector3> pts;
    for (int i = 0; i < 50000; i++) {
        const float t = (float)i;
        pts.push_back(Vector3(-1.6f + std::fmod(t * 0.3713f, 3.2f), -1.6f + std::fmod(t * 0.1931f, 3.2f), -1.6f + std::fmod(t * 0.7717f, 3.2f)));
    }
    pts[0] = Vector3(0.0f, -0.0f, 0.0f);
    pts[1] = Vector3(INFINITY, 1.0f, 0.0f);
    pts[2] = Vector3(3e38f, -1e-45f, NAN);
    std::vector<Vector4> res;
    sdf.Sample(pts, res);
    const int32_t n = (int32_t)ops.size();
    FILE* f = fopen((dir + "/" + name + ".ops").c_str(), "wb");
    fwrite(&n, 4, 1, f); fwrite(out, 4, 4, f); fwrite(ops.data(), sizeof(sdfk_op), ops.size(), f); fclose(f);
    f = fopen((dir + "/" + name + ".pts").c_str(), "wb");
    fwrite(pts.data(), sizeof(Vector3), pts.size(), f); fclose(f);
    f = fopen((dir + "/" + name + ".out").c_str(), "wb");
    fwrite(res.data(), sizeof(Vector4), res.size(), f); fclose(f);
}

static void ElidedIsStored(const Sdf& s)
{
    SetOption(SDFK_OPT_ELIDE_VOLUME, 0);
    Mesh a = s.ToMesh(Vector3(-1.5f), Vector3(1.5f), 136, 132, 128);
    SetOption(SDFK_OPT_ELIDE_VOLUME, 2);
    Mesh b = s.ToMesh(Vector3(-1.5f), Vector3(1.5f), 136, 132, 128);
    IS_TRUE(a.Vertices.size() > 1000);
    IS_TRUE(a.Triangles == b.Triangles);
    bool same = a.Vertices.size() == b.Vertices.size();
    for (size_t i = 0; same && i < a.Vertices.size(); i++)
        same = a.Vertices[i].X == b.Vertices[i].X && a.Vertices[i].Y == b.Vertices[i].Y && a.Vertices[i].Z == b.Vertices[i].Z &&
               a.Colors[i].X == b.Colors[i].X && a.Colors[i].Y == b.Colors[i].Y && a.Colors[i].Z == b.Colors[i].Z;
    IS_TRUE(same);
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s OUTDIR\n", argv[0]); return 2; }
    bool threw = false;
    try { (void)MathF::Sin(Val(1.0f)); } catch (const std::logic_error&) { threw = true; }
    g_run++; IS_TRUE(threw);                                  // (a literal alone is not a program)
    const Sdf gyroid(Gyroid, true), twist(Twist, true);
    g_run++; printf("Gyroid\n"); Dump(argv[1], "gyroid", gyroid); ElidedIsStored(gyroid);
    g_run++; printf("Twist\n"); Dump(argv[1], "twist", twist); ElidedIsStored(twist);
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
