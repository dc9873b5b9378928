// icp_plane_suite.cpp -- the point-to-plane members of SdfKit::IterativeClosestPoint (include/SdfKit.hpp) against the C ABI:
// RegisterPoints with StaticNormals set reproduces sdfk_icp_register_plane's total, points, iteration count and stats bit for bit
// on a height-field case, Metric::Point stays sdfk_icp_register, and the StaticNormals / AddStaticPoints rules hold.  Runs on the
// GPU through libsdfkit_hip.so (tests/test_gpu_icp_plane_cpp.py builds it).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define IS_TRUE(x) do { if (!(x)) { printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); g_fail++; } } while (0)
#define THROWS(stmt) do { bool threw = false; try { stmt; } catch (const std::invalid_argument&) { threw = true; } IS_TRUE(threw); } while (0)
#define TEST(name) static void name(); static void run_##name() { g_run++; printf("%s\n", #name); name(); } static void name()

static float height(float x, float y) { return 0.25f * std::sin(3.0f * x) * std::cos(2.0f * y) + 0.1f * x * y; }

// a 24 x 24 grid of the height field with its normals, and 200 surface points between the samples, moved a little
static void make_case(std::vector<Vector3>& S, std::vector<Vector3>& Nn, std::vector<Vector3>& D)
{
    const int m = 24;
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) {
            const float x = -1.0f + 2.0f * i / (m - 1), y = -1.0f + 2.0f * j / (m - 1);
            const float fx = 0.75f * std::cos(3.0f * x) * std::cos(2.0f * y) + 0.1f * y, fy = -0.5f * std::sin(3.0f * x) * std::sin(2.0f * y) + 0.1f * x;
            const float l = std::sqrt(fx * fx + fy * fy + 1.0f);
            S.push_back(Vector3(x, y, height(x, y)));
            Nn.push_back(Vector3(-fx / l, -fy / l, 1.0f / l));
        }
    const Matrix4x4 move = Matrix4x4::CreateRotationX(0.02f) * Matrix4x4::CreateTranslation(0.02f, -0.01f, 0.015f);
    unsigned s = 12345u;
    for (int k = 0; k < 200; k++) {
        s = s * 1664525u + 1013904223u;
        const float x = -0.8f + 1.6f * (float)(s >> 8) / 16777216.0f;
        s = s * 1664525u + 1013904223u;
        const float y = -0.8f + 1.6f * (float)(s >> 8) / 16777216.0f;
        D.push_back(Matrix4x4::Transform(Vector3(x, y, height(x, y)), move));
    }
}

static bool same(const void* a, const void* b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }

TEST(PlaneMembersReproduceTheAbi)
{
    std::vector<Vector3> S, Nn, D;
    make_case(S, Nn, D);
    IterativeClosestPoint icp(S);
    IS_TRUE(!icp.HasStaticNormals() && !icp.LastStats.Valid);
    std::vector<Vector3> pointPts = D;
    const Matrix4x4 pointTotal = icp.RegisterPoints(pointPts);
    const int pointIters = icp.Iterations;
    IS_TRUE(!icp.LastStats.Valid);

    icp.SetStaticNormals(Nn);
    std::vector<Vector3> pts = D;
    const Matrix4x4 total = icp.RegisterPoints(pts);
    IS_TRUE(icp.LastStats.Valid && icp.LastStats.Converged && icp.LastStats.Retained == 6 && icp.LastStats.Kept > 100);
    IS_TRUE(icp.Iterations < pointIters);

    const sdfk_icp_params prm{icp.MaxIterations, icp.GoodCorrespondenceDistance, icp.ConvergedMaximumTranslation, icp.ConvergedMaximumRotation};
    std::vector<Vector3> raw = D;
    float rawTotal[16];
    int32_t iters = 0;
    int64_t st[4];
    IS_TRUE(sdfk_icp_register_plane(icp.StaticTree().Handle(), &prm, &Nn[0].X, &raw[0].X, (int64_t)raw.size(), rawTotal, &iters, st) == SDFK_OK);
    IS_TRUE(same(rawTotal, &total.M[0][0], sizeof rawTotal) && same(raw.data(), pts.data(), raw.size() * sizeof(Vector3)) && iters == icp.Iterations);
    double r2;
    std::memcpy(&r2, &st[1], sizeof r2);
    IS_TRUE(st[0] == icp.LastStats.Kept && r2 == icp.LastStats.SumR2 && st[3] == icp.LastStats.Retained);

    std::vector<Vector3> again = D;
    const Matrix4x4 p2 = icp.RegisterPoints(again, IterativeClosestPoint::Metric::Point);
    IS_TRUE(same(&p2.M[0][0], &pointTotal.M[0][0], 16 * sizeof(float)) && same(again.data(), pointPts.data(), again.size() * sizeof(Vector3)));
    IS_TRUE(!icp.LastStats.Valid);
}

TEST(NormalsStayInStep)
{
    std::vector<Vector3> S, Nn, D;
    make_case(S, Nn, D);
    IterativeClosestPoint icp(S);
    THROWS(icp.RegisterPoints(D, IterativeClosestPoint::Metric::Plane));
    THROWS(icp.SetStaticNormals(std::vector<Vector3>(Nn.begin(), Nn.end() - 1)));
    THROWS(icp.AddStaticPoints(D, D));
    icp.SetStaticNormals(Nn);
    THROWS(icp.AddStaticPoints(D));
    THROWS(icp.AddStaticPoints(D, std::vector<Vector3>(3)));
    IS_TRUE(icp.StaticTree().TotalPoints() == (int)S.size());
    icp.AddStaticPoints(std::vector<Vector3>{Vector3(9, 9, 9)}, std::vector<Vector3>{Vector3(0, 0, 1)});
    IS_TRUE(icp.StaticTree().TotalPoints() == (int)S.size() + 1 && icp.StaticNormals().size() == S.size() + 1);
    icp.ClearStaticNormals();
    icp.AddStaticPoints(std::vector<Vector3>{Vector3(8, 8, 8)});
    IS_TRUE(icp.StaticTree().TotalPoints() == (int)S.size() + 2);
}

int main()
{
    run_PlaneMembersReproduceTheAbi(); run_NormalsStayInStep();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
