// raymarch_suite.cpp -- SdfKit::RayMarcher of the C++ host layer (include/SdfKit.hpp) against the oracle's images, bit for bit: four
// scenes built here in C++, rendered through the marcher's public properties (ViewTransform, VerticalFieldOfViewDegrees,
// NearPlaneDistance, FarPlaneDistance, DepthIterations) under the cameras, lenses, shapes and iteration counts that
// tests/test_gpu_raymarch_cpp.py hands over with the oracle's depth and colour of every case.  The vectors are written at run time,
// never recorded: they depend on the host's tanf, which the oracle and this header share on whichever machine runs them.  Runs on the
// GPU through libsdfkit_hip.so.
//
// File (little endian): i64 cases; per case: i32 scene, width, height, iterations; f32 position[3], target[3], up[3], field of view
// in degrees, near, far; the oracle's depth (width x height f32, row-major) and colour (3 per pixel).
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
    int32_t scene = 0, w = 0, h = 0, iters = 0;
    float v[12] = {};
    std::vector<float> depth, rgb;
};
static std::vector<Case> Cases;

static void load(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    int64_t cases = 0;
    bool ok = fread(&cases, sizeof cases, 1, f) == 1;
    Cases.resize(ok ? (size_t)cases : 0);
    for (Case& c : Cases) {
        int32_t h[4];
        ok = ok && fread(h, sizeof h, 1, f) == 1 && fread(c.v, sizeof c.v, 1, f) == 1;
        if (!ok) break;
        c.scene = h[0]; c.w = h[1]; c.h = h[2]; c.iters = h[3];
        const size_t n = (size_t)c.w * c.h;
        c.depth.resize(n); c.rgb.resize(3 * n);
        ok = fread(c.depth.data(), sizeof(float), n, f) == n && fread(c.rgb.data(), sizeof(float), 3 * n, f) == 3 * n;
    }
    fclose(f);
    if (!ok) { printf("short vector file\n"); exit(2); }
}

// every float as bits, all NaNs counting as equal (the payload and sign of a produced NaN differ between x86 and the GPU)
static size_t differing(const std::vector<float>& got, const std::vector<float>& want)
{
    if (got.size() != want.size()) return (size_t)-1;
    size_t bad = 0;
    for (size_t i = 0; i < got.size(); i++) {
        uint32_t a, b;
        memcpy(&a, &got[i], 4); memcpy(&b, &want[i], 4);
        bad += !(a == b || (got[i] != got[i] && want[i] != want[i]));
    }
    return bad;
}

static int render_cases(int scene, const Sdf& sdf)
{
    int seen = 0;
    for (const Case& c : Cases) {
        if (c.scene != scene) continue;
        seen++;
        RayMarcher rm(c.w, c.h, sdf);
        rm.ViewTransform = Matrix4x4::CreateLookAt(Vector3(c.v[0], c.v[1], c.v[2]), Vector3(c.v[3], c.v[4], c.v[5]), Vector3(c.v[6], c.v[7], c.v[8]));
        rm.VerticalFieldOfViewDegrees = c.v[9];
        rm.NearPlaneDistance = c.v[10];
        rm.FarPlaneDistance = c.v[11];
        rm.DepthIterations = c.iters;
        const FloatData d = rm.RenderDepth();
        const Vec3Data img = rm.Render();
        CHECK(d.Width == c.w && d.Height == c.h && img.Width == c.w && img.Height == c.h);
        const size_t bd = differing(d.Values, c.depth), bc = differing(img.Values, c.rgb);
        if (bd || bc)
            printf("  scene %d %dx%d, %d steps, camera (%g %g %g), lens (%g %g %g): %zu depths and %zu colour floats differ\n", scene, c.w, c.h,
                   c.iters, c.v[0], c.v[1], c.v[2], c.v[9], c.v[10], c.v[11], bd, bc);
        CHECK(bd == 0);
        CHECK(bc == 0);
    }
    return seen;
}

TEST(Sphere) { CHECK(render_cases(0, Sdfs::Sphere(1.0f)) == 24); }

TEST(Box) { CHECK(render_cases(1, Sdfs::Box(1.0f)) == 24); }

TEST(ReadmeSceneRepeatXY)   // README.md:24-30 through the expression API, as tests/cpp/reference_suite.cpp builds it
{
    auto sdf = SdfExprs::Sphere(0.5f)
                   .RepeatXY(1.125f, 1.125f, [](Vec3 i, Vec3, Vec4) { return Val(0.9f) * Vec3(Vector3::One()) - Vec3::Abs(i) / Val(6.0f); })
                   .ToSdf();
    CHECK(render_cases(2, sdf) == 24);
}

TEST(UnionOfThree)
{
    auto sdf = SdfExprs::Union(SdfExprs::Sphere(0.6f).Translate(-1, 0, 0),
                               SdfExprs::Union(SdfExprs::Box(0.5f).Translate(1, 0, 0), SdfExprs::Cylinder(0.4f, 0.6f))).ToSdf();
    CHECK(render_cases(3, sdf) == 24);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: raymarch_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_Sphere(); run_Box(); run_ReadmeSceneRepeatXY(); run_UnionOfThree();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
