// mesh_winding_suite.cpp -- SdfKit::MeshSdf::WindingNumber / Contains / ToVoxels(MeshSign) and Mesh::WindingNumber / Contains of
// include/SdfKit.hpp against vectors written by the numpy model (tests/test_gpu_mesh_winding_cpp.py), bit for bit.
// usage: mesh_winding_suite vectors.bin
//   int64 cases; per case: int64 nv, nt, n; f32 V[3 nv]; int32 T[3 nt]; f32 Q[3 n]; uint32 winding[n]; uint8 inside[n]
//   int64 volumes; per volume: int64 nv, nt, nx, ny, nz; f32 min[3], max[3], band; f32 V[3 nv]; int32 T[3 nt];
//                              uint32 parity values[nx ny nz]; uint32 winding values[nx ny nz]
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

static std::vector<Vector3> points(FILE* f, size_t n)
{
    const std::vector<float> v = take<float>(f, 3 * n);
    std::vector<Vector3> p(n);
    if (n) memcpy(&p[0].X, v.data(), 12 * n);
    return p;
}

static bool volume_is(Voxels& v, const std::vector<uint32_t>& want)
{
    size_t k = 0;
    for (int i = 0; i < v.NX; i++)
        for (int j = 0; j < v.NY; j++)
            for (int l = 0; l < v.NZ; l++, k++) {
                const float x = v(i, j, l);
                if (memcmp(&x, &want[k], 4) != 0) return false;
            }
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int64_t cases = take<int64_t>(f, 1)[0];
    for (int64_t k = 0; k < cases; k++) {
        bool failed = false;
        const std::vector<int64_t> h = take<int64_t>(f, 3);
        const size_t n = (size_t)h[2];
        const std::vector<Vector3> V = points(f, (size_t)h[0]);
        const std::vector<int32_t> T = take<int32_t>(f, 3 * (size_t)h[1]);
        const std::vector<Vector3> Q = points(f, n);
        const std::vector<uint32_t> w = take<uint32_t>(f, n);
        const std::vector<uint8_t> inside = take<uint8_t>(f, n);
        MeshSdf sdf(V, T);
        const std::vector<float> got = sdf.WindingNumber(Q);
        EXPECT(got.size() == n && same_bits(got.data(), w.data(), n));
        const std::vector<bool> in = sdf.Contains(Q);
        for (size_t i = 0; i < n; i++) EXPECT(in[i] == (inside[i] != 0));
        EXPECT(same_bits(sdf.WindingNumber(Q, DefaultWindingBeta).data(), w.data(), n));   // the handle again: the hierarchy is kept
        Mesh m;
        m.Vertices = V;
        m.Triangles = T;
        m.Colors.assign(V.size(), Vector3(0, 0, 0));
        m.Normals.assign(V.size(), Vector3(0, 0, 0));
        EXPECT(same_bits(m.WindingNumber(Q).data(), w.data(), n));
        EXPECT(m.Contains(Q) == in);
        g_tests++;
        g_failures += failed;
    }
    const int64_t volumes = take<int64_t>(f, 1)[0];
    for (int64_t k = 0; k < volumes; k++) {
        bool failed = false;
        const std::vector<int64_t> h = take<int64_t>(f, 5);
        const std::vector<float> r = take<float>(f, 7);
        const std::vector<Vector3> V = points(f, (size_t)h[0]);
        const std::vector<int32_t> T = take<int32_t>(f, 3 * (size_t)h[1]);
        const size_t cells = (size_t)(h[2] * h[3] * h[4]);
        const std::vector<uint32_t> parity = take<uint32_t>(f, cells), winding = take<uint32_t>(f, cells);
        const Vector3 mn(r[0], r[1], r[2]), mx(r[3], r[4], r[5]);
        MeshSdf sdf(V, T);
        Voxels p = sdf.ToVoxels(mn, mx, (int)h[2], (int)h[3], (int)h[4], r[6]);
        Voxels p2 = sdf.ToVoxels(mn, mx, (int)h[2], (int)h[3], (int)h[4], r[6], false, MeshSign::Parity);
        Voxels w = sdf.ToVoxels(mn, mx, (int)h[2], (int)h[3], (int)h[4], r[6], false, MeshSign::Winding);
        EXPECT(volume_is(p, parity));
        EXPECT(volume_is(p2, parity));
        EXPECT(volume_is(w, winding));
        Voxels again(mn, mx, (int)h[2], (int)h[3], (int)h[4]);
        sdf.SampleInto(again, r[6], MeshSign::Winding, DefaultWindingBeta);
        EXPECT(volume_is(again, winding));
        g_tests++;
        g_failures += failed;
    }
    fclose(f);
    printf("%d tests, %d failures\n", g_tests, g_failures);
    return g_failures ? 1 : 0;
}
