// points_normals_host.cpp -- sdfkit_amd/csrc/points_normals.h built for the host (g++ -ffp-contract=off): covariance, the Jacobi
// eigen step, orientation, the blend of tangent-plane distances and the far fill as the kernels of lib_pointcloud.hip run them,
// driven by tests/test_pointcloud.py, which compares every answer with tests/pointcloud_model.py bit for bit.
//
//   points_normals_host normals IN OUT   IN (f32): cases, has_viewpoint, then per case: m, p_i (3), viewpoint (3), 64 neighbours (3 each)
//                                        OUT (f32): per case normal (3), variation
//   points_normals_host blend   IN OUT   IN (f32): cases, k, max_distance, then per case: m, x (3), 64 x (p (3), n (3), d2)
//                                        OUT (f32): per case known (0 / 1), value
//   points_normals_host fill    IN OUT   IN (i32): nx, ny, nz, then nx * ny * nz signs (z fastest) -> OUT (i32): the signs after the
//                                        passes along z, y, x (a volume without a sign: all +1), then the number of entries filled
//   points_normals_host sign    IN OUT   IN (f32): known values -> OUT (i32): the sign each hands to the far fill
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/points_normals.h"

using namespace sdfk_pc;

template <class T>
static std::vector<T> read_all(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)n / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("read"); exit(2); }
    fclose(f);
    return v;
}

template <class T>
static void write_all(const char* path, const std::vector<T>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const char* mode = argv[1];
    if (!strcmp(mode, "normals")) {
        const auto in = read_all<float>(argv[2]);
        const size_t cases = (size_t)in.at(0), stride = 7 + 3 * 64;
        const bool has_view = in.at(1) != 0.0f;
        if (in.size() != 2 + cases * stride) return 2;
        std::vector<float> out;
        for (size_t c = 0; c < cases; c++) {
            const float* r = in.data() + 2 + c * stride;
            const int m = (int)r[0];
            const float* pi = r + 1;
            const float* nb = r + 7;
            Mean mean;
            for (int j = 0; j < m; j++) mean.add(nb + 3 * j, pi);
            if (m > 0) mean.finish(m);
            Cov C;
            for (int j = 0; j < m; j++) C.add(nb + 3 * j, pi, mean);
            float nrm[3], var;
            normal_of(C, m, pi, has_view, r + 4, nrm, &var);
            out.insert(out.end(), nrm, nrm + 3);
            out.push_back(var);
        }
        write_all(argv[3], out);
    } else if (!strcmp(mode, "blend")) {
        const auto in = read_all<float>(argv[2]);
        const size_t cases = (size_t)in.at(0), stride = 4 + 7 * 64;
        const int k = (int)in.at(1);
        const float md = in.at(2);
        if (in.size() != 3 + cases * stride || k < 1 || k > 64) return 2;
        const float bound = sdfk_knn::radius_d2_bound(md);
        std::vector<float> out;
        for (size_t c = 0; c < cases; c++) {
            const float* r = in.data() + 3 + c * stride;
            const int m = (int)r[0];
            const float* x = r + 1;
            const float* nb = r + 4;
            Blend b;
            if (m > 0) {
                const float h2 = cutoff_d2(m, k, nb[7 * (m - 1) + 6], bound);
                for (int j = 0; j < m; j++) b.add(x, nb + 7 * j, nb + 7 * j + 3, nb[7 * j + 6], h2);
            }
            out.push_back(b.known() ? 1.0f : 0.0f);
            out.push_back(b.known() ? b.value(md) : 0.0f);
        }
        write_all(argv[3], out);
    } else if (!strcmp(mode, "fill")) {
        const auto in = read_all<int32_t>(argv[2]);
        const int nx = in.at(0), ny = in.at(1), nz = in.at(2);
        if (in.size() != 3 + (size_t)nx * ny * nz) return 2;
        std::vector<signed char> s(in.begin() + 3, in.end());
        int filled = 0;
        auto count = [&](int, int) { filled++; };
        for (int i = 0; i < nx; i++)
            for (int j = 0; j < ny; j++) fill_line(s.data() + ((size_t)i * ny + j) * nz, nz, 1, count);
        for (int i = 0; i < nx; i++)
            for (int k = 0; k < nz; k++) fill_line(s.data() + (size_t)i * ny * nz + k, ny, nz, count);
        for (int j = 0; j < ny; j++)
            for (int k = 0; k < nz; k++)
                if (!fill_line(s.data() + (size_t)j * nz + k, nx, (long long)ny * nz, count))
                    for (int i = 0; i < nx; i++) { s[((size_t)i * ny + j) * nz + k] = 1; filled++; }
        std::vector<int32_t> out(s.begin(), s.end());
        out.push_back(filled);
        write_all(argv[3], out);
    } else if (!strcmp(mode, "sign")) {
        const auto in = read_all<float>(argv[2]);
        std::vector<int32_t> out;
        for (float v : in) out.push_back(sign_of(v));
        write_all(argv[3], out);
    } else
        return 2;
    printf("points_normals_host %s ok\n", mode);
    return 0;
}
