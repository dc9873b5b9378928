// pointcloud_suite.cpp -- SdfKit::KdTree::EstimateNormals / ToVoxels (include/SdfKit.hpp) against vectors that
// tests/test_gpu_pointcloud_cpp.py writes with the numpy model (tests/pointcloud_model.py): every bit of every normal, variation
// and voxel.  Runs on the GPU through libsdfkit_hip.so.
//
// File (little endian): i64 n_static, k_normals, k_volume, nx, ny, nz, known; f32 band, viewpoint (3), min (3), max (3); static xyz;
// model normals (n x 3) and variation (n) for the viewpoint; volume normals (n x 3); model volume (nx * ny * nz, z fastest).
#include <cstdio>
#include <cstring>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define CHECK(cond)                                                                                     \
    do { if (!(cond)) { printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } } while (0)
#define TEST(name) static void name(); static void run_##name() { g_run++; printf("%s\n", #name); name(); } static void name()

struct Vectors {
    int64_t n = 0, k_normals = 0, k_volume = 0, nx = 0, ny = 0, nz = 0, known = 0;
    float band = 0;
    Vector3 view, mn, mx;
    std::vector<Vector3> P, normals, volume_normals;
    std::vector<float> variation, volume;
};
static Vectors V;

template <class T>
static void read_vec(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { printf("short vector file\n"); exit(2); }
}

static void load(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    int64_t h[7];
    float r[10];
    if (fread(h, sizeof h, 1, f) != 1 || fread(r, sizeof r, 1, f) != 1) { printf("short vector file\n"); exit(2); }
    V.n = h[0]; V.k_normals = h[1]; V.k_volume = h[2]; V.nx = h[3]; V.ny = h[4]; V.nz = h[5]; V.known = h[6];
    V.band = r[0];
    V.view = Vector3(r[1], r[2], r[3]); V.mn = Vector3(r[4], r[5], r[6]); V.mx = Vector3(r[7], r[8], r[9]);
    read_vec(f, V.P, (size_t)V.n);
    read_vec(f, V.normals, (size_t)V.n);
    read_vec(f, V.variation, (size_t)V.n);
    read_vec(f, V.volume_normals, (size_t)V.n);
    read_vec(f, V.volume, (size_t)(V.nx * V.ny * V.nz));
    fclose(f);
}

template <class T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

TEST(NormalsEqualTheModel)
{
    KdTree tree(V.P);
    const KdTree::Normals r = tree.EstimateNormals((int)V.k_normals, V.view);
    CHECK(same_bits(r.Normal, V.normals));
    CHECK(same_bits(r.Variation, V.variation));
}

TEST(VolumeEqualsTheModel)
{
    KdTree tree(V.P);
    KdTree::VolumeStats st;
    Voxels v = tree.ToVoxels(V.volume_normals, V.mn, V.mx, (int)V.nx, (int)V.ny, (int)V.nz, (int)V.k_volume, V.band, false, &st);
    CHECK(st.Known == V.known && st.Known + st.Unknown == V.nx * V.ny * V.nz);
    std::vector<float> got((size_t)(V.nx * V.ny * V.nz));
    for (int i = 0; i < V.nx; i++)
        for (int j = 0; j < V.ny; j++)
            for (int k = 0; k < V.nz; k++) got[((size_t)i * V.ny + j) * V.nz + k] = v(i, j, k);
    CHECK(same_bits(got, V.volume));
    // into an existing volume: the same values
    Voxels w(V.mn, V.mx, (int)V.nx, (int)V.ny, (int)V.nz);
    tree.SampleInto(w, V.volume_normals, (int)V.k_volume, V.band);
    CHECK(memcmp(&w(0, 0, 0), &got[0], 4) == 0 && memcmp(&w((int)V.nx - 1, (int)V.ny - 1, (int)V.nz - 1), &got.back(), 4) == 0);
}

TEST(PlaneAndRefusals)
{
    std::vector<Vector3> plane;
    for (int x = 0; x < 8; x++)
        for (int y = 0; y < 8; y++) plane.push_back(Vector3((float)x, (float)y, 2.0f));
    KdTree tree(plane);
    const KdTree::Normals up = tree.EstimateNormals(8);
    const KdTree::Normals down = tree.EstimateNormals(8, Vector3(3.0f, 3.0f, -5.0f));
    for (size_t i = 0; i < plane.size(); i++) {
        CHECK(up.Normal[i].X == 0 && up.Normal[i].Y == 0 && up.Normal[i].Z == 1 && up.Variation[i] == 0);
        CHECK(down.Normal[i].X == 0 && down.Normal[i].Y == 0 && down.Normal[i].Z == -1);
        if (g_fail) break;
    }
    int refused = 0;
    try { tree.EstimateNormals(2); } catch (const std::exception&) { refused++; }
    try { tree.EstimateNormals(65); } catch (const std::exception&) { refused++; }
    try { tree.ToVoxels(up.Normal, Vector3(0, 0, 0), Vector3(1, 1, 1), 4, 4, 4, 0); } catch (const std::exception&) { refused++; }
    try { tree.ToVoxels(up.Normal, Vector3(0, 0, 0), Vector3(1, 1, 1), 4, 4, 4, 8, 0.0f); } catch (const std::exception&) { refused++; }
    try { tree.ToVoxels({}, Vector3(0, 0, 0), Vector3(1, 1, 1), 4, 4, 4); } catch (const std::exception&) { refused++; }
    CHECK(refused == 5);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: pointcloud_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_NormalsEqualTheModel(); run_VolumeEqualsTheModel(); run_PlaneAndRefusals();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
