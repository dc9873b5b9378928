// mesh_ray_suite.cpp -- SdfKit::MeshSdf::RayCast / Occluded / Render / RenderDepth / RenderTriangles and Mesh::RayCast / Occluded /
// ToImage of include/SdfKit.hpp against vectors written by the numpy model (tests/test_gpu_mesh_ray_cpp.py), bit for bit.
// usage: mesh_ray_suite vectors.bin
//   int64 casts; per cast: int64 nv, nt, has_colors, n; f32 tmin, tmax; f32 V[3 nv]; int32 T[3 nt]; f32 colours[3 nv] when has_colors;
//                          f32 O[3 n]; f32 D[3 n]; int32 triangle[n]; uint32 distance[n]; uint32 weights[3 n]
//   int64 renders; per render: int64 nv, nt, has_colors, width, height; f32 near, far, position[3], target[3], up[3]; the mesh as above;
//                              uint32 depth[w h]; uint32 rgb[3 w h]; int32 triangle[w h]
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

static bool same_bits(const float* a, const uint32_t* b, size_t n) { return n == 0 || memcmp(a, b, 4 * n) == 0; }

template <class T>
static std::vector<T> take(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { printf("short vectors file\n"); exit(3); }
    return v;
}

struct MeshIn {
    std::vector<Vector3> V, C;
    std::vector<int32_t> T;
};

static MeshIn mesh_in(FILE* f, int64_t nv, int64_t nt, int64_t has_colors)
{
    MeshIn m;
    const std::vector<float> v = take<float>(f, 3 * nv);
    m.T = take<int32_t>(f, 3 * nt);
    m.V.resize(nv);
    if (nv) memcpy(&m.V[0].X, v.data(), 12 * nv);
    if (has_colors) {
        const std::vector<float> c = take<float>(f, 3 * nv);
        m.C.resize(nv);
        memcpy(&m.C[0].X, c.data(), 12 * nv);
    }
    return m;
}

static Mesh as_mesh(const MeshIn& in)
{
    Mesh m;
    m.Vertices = in.V;
    m.Triangles = in.T;
    m.Colors = in.C.empty() ? std::vector<Vector3>(in.V.size(), Vector3(0, 0, 0)) : in.C;
    m.Normals.assign(in.V.size(), Vector3(0, 0, 0));
    return m;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int64_t casts = take<int64_t>(f, 1)[0];
    for (int64_t k = 0; k < casts; k++) {
        bool failed = false;
        const std::vector<int64_t> h = take<int64_t>(f, 4);
        const std::vector<float> r = take<float>(f, 2);
        const MeshIn in = mesh_in(f, h[0], h[1], h[2]);
        const size_t n = (size_t)h[3];
        const std::vector<float> o = take<float>(f, 3 * n), d = take<float>(f, 3 * n);
        const std::vector<int32_t> tri = take<int32_t>(f, n);
        const std::vector<uint32_t> dist = take<uint32_t>(f, n), w = take<uint32_t>(f, 3 * n);
        std::vector<Vector3> O(n), D(n);
        if (n) { memcpy(&O[0].X, o.data(), 12 * n); memcpy(&D[0].X, d.data(), 12 * n); }
        MeshSdf sdf(in.V, in.T, in.C);
        const MeshRayHits hits = sdf.RayCast(O, D, r[0], r[1]);
        EXPECT(hits.Triangles == tri);
        EXPECT(same_bits(hits.Distances.data(), dist.data(), n));
        EXPECT(n == 0 || same_bits(&hits.Weights[0].X, w.data(), 3 * n));
        const std::vector<bool> occ = sdf.Occluded(O, D, r[0], r[1]);
        size_t nh = 0;
        for (size_t i = 0; i < n; i++) {
            EXPECT(occ[i] == (tri[i] >= 0) && hits.Hit(i) == occ[i]);
            nh += tri[i] >= 0;
        }
        EXPECT(hits.Points().size() == nh);
        const Mesh m = as_mesh(in);
        const MeshRayHits viaMesh = m.RayCast(O, D, r[0], r[1]);
        EXPECT(viaMesh.Triangles == tri && same_bits(viaMesh.Distances.data(), dist.data(), n));
        EXPECT(m.Occluded(O, D, r[0], r[1]) == occ);
        g_tests++;
        g_failures += failed;
    }
    const int64_t renders = take<int64_t>(f, 1)[0];
    for (int64_t k = 0; k < renders; k++) {
        bool failed = false;
        const std::vector<int64_t> h = take<int64_t>(f, 5);
        const std::vector<float> r = take<float>(f, 11);
        const MeshIn in = mesh_in(f, h[0], h[1], h[2]);
        const int width = (int)h[3], height = (int)h[4];
        const size_t px = (size_t)width * height;
        const std::vector<uint32_t> depth = take<uint32_t>(f, px), rgb = take<uint32_t>(f, 3 * px);
        const std::vector<int32_t> tri = take<int32_t>(f, px);
        const Matrix4x4 view = Matrix4x4::CreateLookAt(Vector3(r[2], r[3], r[4]), Vector3(r[5], r[6], r[7]), Vector3(r[8], r[9], r[10]));
        MeshSdf sdf(in.V, in.T, in.C);
        const FloatData dd = sdf.RenderDepth(width, height, view, 60.0f, r[0], r[1]);
        const Vec3Data cc = sdf.Render(width, height, view, 60.0f, r[0], r[1]);
        EXPECT(dd.Width == width && dd.Height == height && same_bits(dd.Values.data(), depth.data(), px));
        EXPECT(cc.Width == width && cc.Height == height && same_bits(cc.Values.data(), rgb.data(), 3 * px));
        EXPECT(sdf.RenderTriangles(width, height, view, 60.0f, r[0], r[1]) == tri);
        const Vec3Data img = as_mesh(in).ToImage(width, height, Vector3(r[2], r[3], r[4]), Vector3(r[5], r[6], r[7]), Vector3(r[8], r[9], r[10]), 60.0f, r[0], r[1]);
        EXPECT(same_bits(img.Values.data(), rgb.data(), 3 * px));
        g_tests++;
        g_failures += failed;
    }
    fclose(f);
    printf("%d tests, %d failures\n", g_tests, g_failures);
    return g_failures ? 1 : 0;
}
