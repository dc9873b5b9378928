// points_suite.cpp -- the reference's KdTree and IterativeClosestPoint tests on three points (Tests/KdTreeTests.cs,
// Tests/IterativeClosestPointTests.cs: the cases whose inputs need no System.Random), restated against the C++ host layer
// include/SdfKit.hpp.  Runs on the GPU through libsdfkit_hip.so (tests/test_gpu_points_cpp.py builds it).
#include <cmath>
#include <cstdio>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define ARE_EQUAL(expected, actual)                                                                     \
    do { if (!((expected) == (actual))) { printf("  FAIL %s:%d: expected %s == %s (%g vs %g)\n", __FILE__, __LINE__, #expected, #actual, (double)(expected), (double)(actual)); g_fail++; } } while (0)
#define ARE_EQUAL_TOL(expected, actual, tol)                                                            \
    do { if (!(std::fabs((double)(expected) - (double)(actual)) <= (tol))) { printf("  FAIL %s:%d: |%s - %s| = %g > %g\n", __FILE__, __LINE__, #expected, #actual, std::fabs((double)(expected) - (double)(actual)), (double)(tol)); g_fail++; } } while (0)
#define TEST(name) static void name(); static void run_##name() { g_run++; printf("%s\n", #name); name(); } static void name()

static const std::vector<Vector3> threePoints = {Vector3(0, 0, 1), Vector3(0, 1, 0), Vector3(1, 0, 0)};

TEST(KdTreeThreePoints)   // KdTreeTests.cs:11-22
{
    KdTree tree(threePoints);
    ARE_EQUAL(0, (int)tree.SplitAxis);
    ARE_EQUAL(3, tree.TotalPoints());
    float distance = 0;
    const Vector3 nearest = tree.Search(Vector3(0.0f, 1.5f, 0.0f), distance);
    ARE_EQUAL(0.0f, nearest.X);
    ARE_EQUAL(1.0f, nearest.Y);
    ARE_EQUAL(0.0f, nearest.Z);
    ARE_EQUAL_TOL(0.5f, distance, 1.0e-4f);
}

static void ThreePointsTest(const Matrix4x4& expectedTransform)   // IterativeClosestPointTests.cs PointsTest, keep = 1
{
    IterativeClosestPoint cp(threePoints);
    std::vector<Vector3> transformed;
    for (const Vector3& p : threePoints) transformed.push_back(Matrix4x4::Transform(p, expectedTransform));
    const std::vector<Vector3> copy = transformed;
    const Matrix4x4 invTransform = cp.RegisterPoints(transformed);
    Matrix4x4 transform;
    Matrix4x4::Invert(invTransform, transform);
    const Vector3 t = transform.Translation(), e = expectedTransform.Translation();
    ARE_EQUAL_TOL(e.X, t.X, 1.0e-4f);
    ARE_EQUAL_TOL(e.Y, t.Y, 1.0e-4f);
    ARE_EQUAL_TOL(e.Z, t.Z, 1.0e-4f);
    ARE_EQUAL_TOL(expectedTransform.M[0][0], transform.M[0][0], 1.0e-6f);
    ARE_EQUAL_TOL(expectedTransform.M[1][1], transform.M[1][1], 1.0e-6f);
    ARE_EQUAL_TOL(expectedTransform.M[2][2], transform.M[2][2], 1.0e-6f);
    for (size_t i = 0; i < threePoints.size(); i++) {
        const Vector3 p = threePoints[i], q = transformed[i], r = Matrix4x4::Transform(copy[i], invTransform);
        ARE_EQUAL_TOL(p.X, q.X, 1.0e-4f); ARE_EQUAL_TOL(p.Y, q.Y, 1.0e-4f); ARE_EQUAL_TOL(p.Z, q.Z, 1.0e-4f);
        ARE_EQUAL_TOL(p.X, r.X, 1.0e-4f); ARE_EQUAL_TOL(p.Y, r.Y, 1.0e-4f); ARE_EQUAL_TOL(p.Z, r.Z, 1.0e-4f);
    }
}

static const float kDeg = 1.0f * 3.14159265f / 180.0f;   // 1.0f * MathF.PI / 180.0f

TEST(ThreePointsOffsetX) { ThreePointsTest(Matrix4x4::CreateTranslation(0.1f, 0, 0)); }
TEST(ThreePointsOffsetXYZ) { ThreePointsTest(Matrix4x4::CreateTranslation(0.1f, -0.2f, -0.3f)); }
TEST(ThreePointsRotateY) { ThreePointsTest(Matrix4x4::CreateRotationY(kDeg)); }
TEST(ThreePointsRotateXOffsetY) { ThreePointsTest(Matrix4x4::CreateRotationX(kDeg) * Matrix4x4::CreateTranslation(0, 0.1f, 0)); }
TEST(ThreePointsOffsetZRotateXOffsetY)
{
    ThreePointsTest(Matrix4x4::CreateTranslation(0, 0.0f, 0.1f) * Matrix4x4::CreateRotationX(kDeg) * Matrix4x4::CreateTranslation(0, 0.1f, 0));
}

int main()
{
    run_KdTreeThreePoints(); run_ThreePointsOffsetX(); run_ThreePointsOffsetXYZ(); run_ThreePointsRotateY(); run_ThreePointsRotateXOffsetY();
    run_ThreePointsOffsetZRotateXOffsetY();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
