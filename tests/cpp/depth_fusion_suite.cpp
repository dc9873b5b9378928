// depth_fusion_suite.cpp -- SdfKit::DepthFusion and SdfKit::DepthToPoints of include/SdfKit.hpp against vectors written by the
// numpy model (tests/test_gpu_depth_fusion_cpp.py), bit for bit.
// usage: depth_fusion_suite vectors.bin
//   int64 volumes; per volume: int64 nx, ny, nz, frames, carve; f32 truncation, unseen, max_weight, min[3], max[3];
//       per frame: int64 width, height; f32 weight, depth_min, depth_max, near, position[3], target[3], up[3]; f32 depth[w h]; int64 stats[4];
//       uint32 D[nx ny nz]; uint32 W[nx ny nz]
//   int64 frames; per frame: int64 width, height, has_rgb, n; f32 position[3], target[3], up[3]; f32 depth[w h]; f32 rgb[3 w h] when has_rgb;
//       uint32 points[3 n]; uint32 colors[3 n] when has_rgb; int32 pixel[n]
#include <cstdio>
#include <cstring>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_tests = 0, g_failures = 0;
#define EXPECT(cond)                                                                        \
    do {                                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failed = true; } \
    } while (0)

// equal as bits; a NaN that arithmetic made equals any NaN
static bool same_bits(const float* a, const uint32_t* b, size_t n)
{
    for (size_t k = 0; k < n; k++) {
        uint32_t u;
        memcpy(&u, a + k, 4);
        const bool nan_a = (u & 0x7fffffffu) > 0x7f800000u, nan_b = (b[k] & 0x7fffffffu) > 0x7f800000u;
        if (nan_a != nan_b || (!nan_a && u != b[k])) return false;
    }
    return true;
}

template <class T>
static std::vector<T> take(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { printf("short vectors file\n"); exit(3); }
    return v;
}

static Vector3 v3(const float* p) { return Vector3(p[0], p[1], p[2]); }

static std::vector<float> all_of(Voxels& v)
{
    std::vector<float> out;
    for (int i = 0; i < v.NX; i++)
        for (int j = 0; j < v.NY; j++)
            for (int k = 0; k < v.NZ; k++) out.push_back(v(i, j, k));
    return out;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int64_t volumes = take<int64_t>(f, 1)[0];
    for (int64_t c = 0; c < volumes; c++) {
        bool failed = false;
        const std::vector<int64_t> h = take<int64_t>(f, 5);
        const std::vector<float> q = take<float>(f, 9);
        DepthFusion fu(v3(&q[3]), v3(&q[6]), (int)h[0], (int)h[1], (int)h[2], q[0], q[1], h[4] != 0, q[2]);
        for (int64_t k = 0; k < h[3]; k++) {
            const std::vector<int64_t> wh = take<int64_t>(f, 2);
            const std::vector<float> a = take<float>(f, 13);
            FloatData d;
            d.Width = (int)wh[0]; d.Height = (int)wh[1];
            d.Values = take<float>(f, (size_t)(wh[0] * wh[1]));
            const std::vector<int64_t> want = take<int64_t>(f, 4);
            DepthFusionStats st;
            fu.Integrate(d, v3(&a[4]), v3(&a[7]), v3(&a[10]), a[0], a[1], a[2], &st, 60.0f, a[3], 100.0f);
            EXPECT(st.Updated == want[0] && st.Surface == want[1] && st.First == want[2] && st.ValidPixels == want[3]);
        }
        const size_t n = (size_t)(h[0] * h[1] * h[2]);
        const std::vector<uint32_t> D = take<uint32_t>(f, n), W = take<uint32_t>(f, n);
        EXPECT(fu.Frames == (int)h[3]);
        EXPECT(same_bits(all_of(fu.ToVoxels()).data(), D.data(), n));
        EXPECT(same_bits(all_of(fu.Weights).data(), W.data(), n));
        g_tests++;
        g_failures += failed;
        printf("volume %lld: %s\n", (long long)c, failed ? "FAILED" : "ok");
    }
    const int64_t frames = take<int64_t>(f, 1)[0];
    for (int64_t c = 0; c < frames; c++) {
        bool failed = false;
        const std::vector<int64_t> h = take<int64_t>(f, 4);
        const std::vector<float> a = take<float>(f, 9);
        const size_t npix = (size_t)(h[0] * h[1]), n = (size_t)h[3];
        FloatData d;
        d.Width = (int)h[0]; d.Height = (int)h[1];
        d.Values = take<float>(f, npix);
        Vec3Data rgb;
        rgb.Width = d.Width; rgb.Height = d.Height;
        if (h[2]) rgb.Values = take<float>(f, 3 * npix);
        const std::vector<uint32_t> P = take<uint32_t>(f, 3 * n), C = take<uint32_t>(f, h[2] ? 3 * n : 0);
        const std::vector<int32_t> X = take<int32_t>(f, n);
        const DepthPoints got = DepthToPoints(d, v3(&a[0]), v3(&a[3]), v3(&a[6]), h[2] ? &rgb : nullptr);
        EXPECT(got.Points.size() == n && got.Pixels == X && got.Colors.size() == (h[2] ? n : 0));
        if (!failed && n) {
            EXPECT(same_bits(&got.Points[0].X, P.data(), 3 * n));
            if (h[2]) EXPECT(same_bits(&got.Colors[0].X, C.data(), 3 * n));
        }
        g_tests++;
        g_failures += failed;
        printf("frame %lld: %s\n", (long long)c, failed ? "FAILED" : "ok");
    }
    fclose(f);
    printf("%d tests, %d failures\n", g_tests, g_failures);
    return g_failures ? 1 : 0;
}
