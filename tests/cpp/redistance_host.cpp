// Host build of sdfkit_amd/csrc/redistance.h (the functions the kernels of lib_redistance.hip call) as a full-sweep Jacobi
// solver: every voxel in every sweep, double-buffered, until a sweep changes nothing -- no tiles, no active set.
//   redistance_host IN OUT     IN: int32 nx ny nz, f32 hx hy hz iso band, then nx*ny*nz f32 values (z fastest)
//                              OUT: nx*ny*nz f32 result, then int64 sweeps, 0, front voxels, clamped voxels
// g++ -std=c++17 -O2 -ffp-contract=off -pthread
#include "../../sdfkit_amd/csrc/redistance.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

using namespace sdfk_redistance;

template <typename F>
static void parallel_x(int nx, F f)
{
    const int nt = std::max(1, std::min({(int)std::thread::hardware_concurrency(), 16, nx}));
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back([=] { f(nx * t / nt, nx * (t + 1) / nt); });
    for (auto& t : th) t.join();
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n[3];
    float par[5];
    if (fread(n, 4, 3, f) != 3 || fread(par, 4, 5, f) != 5) return 2;
    const int nx = n[0], ny = n[1], nz = n[2];
    const size_t nv = (size_t)nx * ny * nz;
    std::vector<float> v(nv);
    if (fread(v.data(), 4, nv, f) != nv) return 2;
    fclose(f);
    const double h[3] = {(double)par[0], (double)par[1], (double)par[2]};
    const double iso = (double)par[3];
    const float band = par[4];
    const size_t stride[3] = {(size_t)ny * nz, (size_t)nz, 1};

    std::vector<float> T(nv), U(nv);
    std::vector<uint8_t> frozen(nv);
    std::atomic<long long> nfront{0};
    parallel_x(nx, [&](int x0, int x1) {
        long long c = 0;
        for (int x = x0; x < x1; x++)
            for (int y = 0; y < ny; y++)
                for (int z = 0; z < nz; z++) {
                    const int p[3] = {x, y, z};
                    const size_t o = ((size_t)x * ny + y) * nz + z;
                    double sn[6];
                    bool in[6];
                    for (int a = 0; a < 3; a++) {
                        in[2 * a] = p[a] > 0;
                        in[2 * a + 1] = p[a] + 1 < n[a];
                        sn[2 * a] = in[2 * a] ? (double)v[o - stride[a]] - iso : 0.0;
                        sn[2 * a + 1] = in[2 * a + 1] ? (double)v[o + stride[a]] - iso : 0.0;
                    }
                    float t0;
                    frozen[o] = rd_front((double)v[o] - iso, sn, in, h, &t0) ? 1 : 0;
                    T[o] = frozen[o] ? t0 : INFINITY;
                    c += frozen[o];
                }
        nfront += c;
    });
    long long sweeps = 0;
    if (nfront > 0)
        for (;;) {
            std::atomic<int> changed{0};
            parallel_x(nx, [&](int x0, int x1) {
                int ch = 0;
                for (int x = x0; x < x1; x++)
                    for (int y = 0; y < ny; y++)
                        for (int z = 0; z < nz; z++) {
                            const int p[3] = {x, y, z};
                            const size_t o = ((size_t)x * ny + y) * nz + z;
                            float out = T[o];
                            if (!frozen[o]) {
                                float tn[6];
                                for (int a = 0; a < 3; a++) {
                                    tn[2 * a] = p[a] > 0 ? T[o - stride[a]] : INFINITY;
                                    tn[2 * a + 1] = p[a] + 1 < n[a] ? T[o + stride[a]] : INFINITY;
                                }
                                out = rd_sweep_voxel(T[o], tn, h, band);
                                ch |= out != T[o];
                            }
                            U[o] = out;
                        }
                if (ch) changed = 1;
            });
            sweeps++;
            if (!changed) break;
            T.swap(U);
        }
    long long clamped = 0;
    for (size_t o = 0; o < nv; o++) {
        clamped += T[o] > band;
        U[o] = rd_finish(T[o], (double)v[o] - iso, band);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const int64_t stats[4] = {sweeps, 0, nfront.load(), clamped};
    fwrite(U.data(), 4, nv, f);
    fwrite(stats, 8, 4, f);
    fclose(f);
    printf("redistance ok %lld sweeps\n", sweeps);
    return 0;
}
