// pointcloud_color_suite.cpp -- SdfKit::KdTree::SampleColors, ToVoxels with colours and VoxelDownsample with colours
// (include/SdfKit.hpp) against vectors that tests/test_gpu_pointcloud_color_cpp.py writes with the numpy model
// (tests/pointcloud_color_model.py): every bit of every colour.  Runs on the GPU through libsdfkit_hip.so.
//
// File (little endian): i64 n_static, n_queries, k_sample, k_volume, nx, ny, nz, known, m; f32 sample_distance, band, voxel_size,
// min (3), max (3); static xyz; colours (n x 3); normals (n x 3); queries; model colours at the queries (q x 3) and found (q x i32);
// model volume (nx * ny * nz, z fastest) and its colours (x 3); model downsampled points (m x 3), counts (m x i32), group
// (n x i32), colours (m x 3).
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
    int64_t n = 0, nq = 0, k_sample = 0, k_volume = 0, nx = 0, ny = 0, nz = 0, known = 0, m = 0;
    float sample_distance = 0, band = 0, voxel_size = 0;
    Vector3 mn, mx;
    std::vector<Vector3> P, colors, normals, Q, sampled, volume_colors, down_points, down_colors;
    std::vector<int32_t> found, down_counts, down_group;
    std::vector<float> volume;
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
    int64_t h[9];
    float r[9];
    if (fread(h, sizeof h, 1, f) != 1 || fread(r, sizeof r, 1, f) != 1) { printf("short vector file\n"); exit(2); }
    V.n = h[0]; V.nq = h[1]; V.k_sample = h[2]; V.k_volume = h[3]; V.nx = h[4]; V.ny = h[5]; V.nz = h[6]; V.known = h[7]; V.m = h[8];
    V.sample_distance = r[0]; V.band = r[1]; V.voxel_size = r[2];
    V.mn = Vector3(r[3], r[4], r[5]); V.mx = Vector3(r[6], r[7], r[8]);
    const size_t nvox = (size_t)(V.nx * V.ny * V.nz);
    read_vec(f, V.P, (size_t)V.n);
    read_vec(f, V.colors, (size_t)V.n);
    read_vec(f, V.normals, (size_t)V.n);
    read_vec(f, V.Q, (size_t)V.nq);
    read_vec(f, V.sampled, (size_t)V.nq);
    read_vec(f, V.found, (size_t)V.nq);
    read_vec(f, V.volume, nvox);
    read_vec(f, V.volume_colors, nvox);
    read_vec(f, V.down_points, (size_t)V.m);
    read_vec(f, V.down_counts, (size_t)V.m);
    read_vec(f, V.down_group, (size_t)V.n);
    read_vec(f, V.down_colors, (size_t)V.m);
    fclose(f);
}

template <class T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

TEST(SampleColorsEqualTheModel)
{
    KdTree tree(V.P);
    const KdTree::SampledColors r = tree.SampleColors(V.Q, V.colors, (int)V.k_sample, V.sample_distance);
    CHECK(same_bits(r.Colors, V.sampled));
    CHECK(same_bits(r.Found, V.found));
    int refused = 0;
    try { tree.SampleColors(V.Q, V.colors, 0); } catch (const std::exception&) { refused++; }
    try { tree.SampleColors(V.Q, V.colors, 65); } catch (const std::exception&) { refused++; }
    try { tree.SampleColors(V.Q, {}, 8); } catch (const std::exception&) { refused++; }
    CHECK(refused == 3);
}

TEST(ColouredVolumeEqualsTheModel)
{
    KdTree tree(V.P);
    KdTree::VolumeStats st;
    Voxels v = tree.ToVoxels(V.normals, V.colors, V.mn, V.mx, (int)V.nx, (int)V.ny, (int)V.nz, (int)V.k_volume, V.band, false, &st);
    CHECK(st.Known == V.known && st.Known + st.Unknown == V.nx * V.ny * V.nz);
    std::vector<float> values(V.volume.size());
    std::vector<Vector3> colors(V.volume_colors.size());
    Check(sdfk_volume_download(v.Sync(), values.data(), &colors[0].X));
    CHECK(same_bits(values, V.volume));
    CHECK(same_bits(colors, V.volume_colors));
    // into a volume that had no colour storage: the same, and the colourless call then leaves the colours alone
    Voxels w = tree.ToVoxels(V.normals, V.mn, V.mx, (int)V.nx, (int)V.ny, (int)V.nz, 1, V.band);
    tree.SampleInto(w, V.normals, (int)V.k_volume, V.band, nullptr, &V.colors);
    Check(sdfk_volume_download(w.Sync(), values.data(), &colors[0].X));
    CHECK(same_bits(values, V.volume) && same_bits(colors, V.volume_colors));
    tree.SampleInto(w, V.normals, 1, V.band);
    Check(sdfk_volume_download(w.Sync(), values.data(), &colors[0].X));
    CHECK(!same_bits(values, V.volume) && same_bits(colors, V.volume_colors));
    // Redistance copies them
    Voxels full = v.Redistance();
    Check(sdfk_volume_download(full.Sync(), values.data(), &colors[0].X));
    CHECK(same_bits(colors, V.volume_colors));
    int refused = 0;
    try { tree.ToVoxels(V.normals, std::vector<Vector3>(3), V.mn, V.mx, 4, 4, 4); } catch (const std::exception&) { refused++; }
    try { tree.ToVoxels(V.normals, V.colors, V.mn, V.mx, 4, 4, 4, 65); } catch (const std::exception&) { refused++; }
    CHECK(refused == 2);
}

TEST(DownsampledColoursEqualTheModel)
{
    KdTree tree(V.P);
    const KdTree::Downsampled r = tree.VoxelDownsample(V.voxel_size, V.colors);
    CHECK(same_bits(r.Colors, V.down_colors));
    CHECK(same_bits(r.Points, V.down_points) && same_bits(r.Counts, V.down_counts) && same_bits(r.Group, V.down_group));
    const KdTree::Downsampled plain = tree.VoxelDownsample(V.voxel_size);
    CHECK(plain.Colors.empty() && same_bits(plain.Points, r.Points) && same_bits(plain.Counts, r.Counts) && same_bits(plain.Group, r.Group));
    int refused = 0;
    try { tree.VoxelDownsample(V.voxel_size, std::vector<Vector3>(3)); } catch (const std::exception&) { refused++; }
    try { tree.VoxelDownsample(0.0f, V.colors); } catch (const std::exception&) { refused++; }
    CHECK(refused == 2);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: pointcloud_color_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_SampleColorsEqualTheModel(); run_ColouredVolumeEqualsTheModel(); run_DownsampledColoursEqualTheModel();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
