// redistance_suite.cpp -- Voxels::Redistance through the C++ host layer include/SdfKit.hpp, bit for bit against a full-sweep
// Jacobi solver built here from the SAME csrc/redistance.h the kernels call (every voxel in every sweep, no tiles, no active
// set): anisotropic non-tile-multiple volumes, an iso value, the band as the clamp of the unbanded run, the refusals, and the
// loop Sdf -> Mesh -> banded Voxels -> Redistance.  Runs on the GPU through libsdfkit_hip.so (tests/test_gpu_redistance_cpp.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "SdfKit.hpp"
#include "../../sdfkit_amd/csrc/redistance.h"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define IS_TRUE(c) do { if (!(c)) { printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)
#define TEST(name) static void name(); static void run_##name() { g_run++; printf("%s\n", #name); name(); } static void name()

static std::vector<float> HostSolve(const std::vector<float>& v, const int n[3], const float hf[3], float isof, float band, long long* sweeps_out)
{
    using namespace sdfk_redistance;
    const double h[3] = {hf[0], hf[1], hf[2]}, iso = isof;
    const size_t stride[3] = {(size_t)n[1] * n[2], (size_t)n[2], 1}, nv = (size_t)n[0] * n[1] * n[2];
    std::vector<float> T(nv), U(nv);
    std::vector<char> frozen(nv);
    bool any = false;
    auto each = [&](auto f) {
        for (int x = 0; x < n[0]; x++) for (int y = 0; y < n[1]; y++) for (int z = 0; z < n[2]; z++) { const int p[3] = {x, y, z}; f(p, ((size_t)x * n[1] + y) * n[2] + z); }
    };
    each([&](const int p[3], size_t o) {
        double sn[6];
        bool in[6];
        for (int a = 0; a < 3; a++) {
            in[2 * a] = p[a] > 0; in[2 * a + 1] = p[a] + 1 < n[a];
            sn[2 * a] = in[2 * a] ? (double)v[o - stride[a]] - iso : 0.0;
            sn[2 * a + 1] = in[2 * a + 1] ? (double)v[o + stride[a]] - iso : 0.0;
        }
        float t0;
        frozen[o] = rd_front((double)v[o] - iso, sn, in, h, &t0);
        T[o] = frozen[o] ? t0 : INFINITY;
        any |= frozen[o];
    });
    long long sweeps = 0;
    while (any) {
        bool changed = false;
        each([&](const int p[3], size_t o) {
            float out = T[o];
            if (!frozen[o]) {
                float tn[6];
                for (int a = 0; a < 3; a++) {
                    tn[2 * a] = p[a] > 0 ? T[o - stride[a]] : INFINITY;
                    tn[2 * a + 1] = p[a] + 1 < n[a] ? T[o + stride[a]] : INFINITY;
                }
                out = rd_sweep_voxel(T[o], tn, h, band);
                changed |= out != T[o];
            }
            U[o] = out;
        });
        sweeps++;
        if (!changed) break;
        T.swap(U);
    }
    for (size_t o = 0; o < nv; o++) U[o] = rd_finish(T[o], (double)v[o] - iso, band);
    if (sweeps_out) *sweeps_out = sweeps;
    return U;
}

// two spheres (a crease between them) scaled by 2.5: the zero set of a distance, not a distance
static float Field(float x, float y, float z)
{
    const float a = std::sqrt((x + 0.4f) * (x + 0.4f) + y * y + z * z) - 0.7f;
    const float b = std::sqrt((x - 0.5f) * (x - 0.5f) + (y - 0.2f) * (y - 0.2f) + (z + 0.1f) * (z + 0.1f)) - 0.55f;
    return 2.5f * std::fmin(a, b);
}

static Voxels Fill(Vector3 mn, Vector3 mx, const int n[3], std::vector<float>& host)
{
    Voxels v(mn, mx, n[0], n[1], n[2]);
    host.assign((size_t)n[0] * n[1] * n[2], 0.0f);
    for (int x = 0; x < n[0]; x++)
        for (int y = 0; y < n[1]; y++)
            for (int z = 0; z < n[2]; z++) {
                const float f = Field(mn.X + v.DX * (x + 0.5f), mn.Y + v.DY * (y + 0.5f), mn.Z + v.DZ * (z + 0.5f));
                v(x, y, z) = f;
                host[((size_t)x * n[1] + y) * n[2] + z] = f;
            }
    return v;
}

static size_t Mismatches(Voxels& got, const std::vector<float>& want, const int n[3])
{
    size_t bad = 0;
    for (int x = 0; x < n[0]; x++)
        for (int y = 0; y < n[1]; y++)
            for (int z = 0; z < n[2]; z++) {
                const float a = got(x, y, z), b = want[((size_t)x * n[1] + y) * n[2] + z];
                bad += std::memcmp(&a, &b, 4) != 0;
            }
    return bad;
}

TEST(EqualsFullSweepHostSolverBitwise)
{
    const int n[3] = {37, 19, 51};
    std::vector<float> host;
    Voxels v = Fill(Vector3(-1.5f, -1.0f, -1.2f), Vector3(1.5f, 1.1f, 1.3f), n, host);
    const float h[3] = {v.DX, v.DY, v.DZ};
    for (float iso : {0.0f, 0.3f}) {
        int64_t st[4];
        Voxels r = v.Redistance(iso, INFINITY, st);
        long long sweeps = 0;
        const std::vector<float> want = HostSolve(host, n, h, iso, INFINITY, &sweeps);
        printf("  iso %g: %lld sweeps, %lld tile-sweeps of %lld, %lld front voxels\n", iso, (long long)st[0], (long long)st[1], (long long)(st[0] * 5 * 3 * 7), (long long)st[2]);
        IS_TRUE(Mismatches(r, want, n) == 0);
        IS_TRUE(st[0] == sweeps && st[2] > 0 && st[3] == 0);
        IS_TRUE(r.NX == n[0] && r.NY == n[1] && r.NZ == n[2] && r.DX == v.DX && r.Version() > 0);
    }
    IS_TRUE(Mismatches(v, host, n) == 0);   // the input is what it was
}

TEST(BandEqualsClampOfUnbanded)
{
    const int n[3] = {40, 24, 56};
    std::vector<float> host;
    Voxels v = Fill(Vector3(-1.5f, -1.0f, -1.2f), Vector3(1.5f, 1.1f, 1.3f), n, host);
    const float band = 3.0f * v.DX;
    Voxels full = v.Redistance();
    int64_t st[4];
    Voxels banded = v.Redistance(0.0f, band, st);
    std::vector<float> clamp(host.size());
    size_t over = 0;
    for (int x = 0; x < n[0]; x++)
        for (int y = 0; y < n[1]; y++)
            for (int z = 0; z < n[2]; z++) {
                const float f = full(x, y, z);
                over += std::fabs(f) > band;
                clamp[((size_t)x * n[1] + y) * n[2] + z] = std::fabs(f) < band ? f : std::copysign(band, f);
            }
    IS_TRUE(Mismatches(banded, clamp, n) == 0);
    IS_TRUE((size_t)st[3] == over && over > 0);
}

TEST(RefusalsThrow)
{
    const int n[3] = {9, 8, 7};
    std::vector<float> host;
    Voxels v = Fill(Vector3(-1), Vector3(1), n, host);
    int thrown = 0;
    try { v.Redistance(0.0f, -1.0f); } catch (const std::exception&) { thrown++; }
    try { v.Redistance(NAN); } catch (const std::exception&) { thrown++; }
    v(3, 3, 3) = NAN;
    try { v.Redistance(); } catch (const std::exception& e) { thrown++; printf("  %s\n", e.what()); }
    IS_TRUE(thrown == 3);
    v(3, 3, 3) = 1.0f;
    Voxels r = v.Redistance();
    IS_TRUE(std::isfinite(r(0, 0, 0)));
}

TEST(BandedMeshVolumeToFullField)
{
    const int N = 64;
    const Vector3 mn(-1.5f), mx(1.5f);
    Mesh mesh = Sdfs::Sphere(1.0f).ToMesh(mn, mx, N, N, N);
    MeshSdf m(mesh);
    const float dx = 3.0f / N;
    Voxels banded = m.ToVoxels(mn, mx, N, N, N, 4 * dx);
    Voxels red = banded.Redistance();
    // the same sign at every voxel => the same sign-changing edges and cell configurations => the same mesh sizes
    Mesh a = banded.ToMesh(), b = red.ToMesh();
    IS_TRUE(a.Vertices.size() == b.Vertices.size() && a.Triangles.size() == b.Triangles.size() && !a.Triangles.empty());
    int bad = 0;
    float worst = 0, flat = 0;
    for (int x = 0; x < N; x++)
        for (int y = 0; y < N; y++)
            for (int z = 0; z < N; z++) {
                const float px = -1.5f + dx * (x + 0.5f), py = -1.5f + dx * (y + 0.5f), pz = -1.5f + dx * (z + 0.5f);
                const float ana = std::sqrt(px * px + py * py + pz * pz) - 1.0f;
                bad += (red(x, y, z) > 0) != (banded(x, y, z) > 0);
                worst = std::fmax(worst, std::fabs(red(x, y, z) - ana) / dx);
                flat = std::fmax(flat, std::fabs(banded(x, y, z) - ana) / dx);
            }
    printf("  far field: banded volume off by up to %.1f voxels, redistanced by %.3f voxels\n", flat, worst);
    IS_TRUE(bad == 0);
    IS_TRUE(worst < 2.0f && flat > 10.0f);   // (first order: about one voxel at this size; the figures are tests/golden/redistance_accuracy.json's)
}

int main()
{
    run_EqualsFullSweepHostSolverBitwise(); run_BandEqualsClampOfUnbanded(); run_RefusalsThrow(); run_BandedMeshVolumeToFullField();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
