// points_color_host.cpp -- sdfkit_amd/csrc/points_color.h built for the host (g++ -ffp-contract=off): the blend of the neighbours'
// colours and the mean colour of a voxel's members as the kernels of lib_pointcloud.hip and lib_points_filter.hip run them, driven
// by tests/test_pointcloud_color.py, which compares every answer with tests/pointcloud_color_model.py bit for bit.
//
//   points_color_host blend IN OUT   IN (f32): cases, k, max_distance, then per case: m, 64 x (colour (3), d2)
//                                    OUT (f32): per case the colour (3)
//   points_color_host mean  IN OUT   IN (f32): groups, then per group: count, count x colour (3) (the members in ascending index)
//                                    OUT (f32): per group the mean colour (3)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/points_color.h"
#include "../../sdfkit_amd/csrc/points_normals.h"

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
    const auto in = read_all<float>(argv[2]);
    std::vector<float> out;
    if (!strcmp(mode, "blend")) {
        const size_t cases = (size_t)in.at(0), stride = 1 + 4 * 64;
        const int k = (int)in.at(1);
        const float md = in.at(2);
        if (in.size() != 3 + cases * stride || k < 1 || k > 64) return 2;
        const float bound = sdfk_knn::radius_d2_bound(md);
        for (size_t c = 0; c < cases; c++) {
            const float* r = in.data() + 3 + c * stride;
            const int m = (int)r[0];
            const float* nb = r + 1;
            sdfk_color::Blend b;
            if (m > 0) {
                const float h2 = sdfk_pc::cutoff_d2(m, k, nb[4 * (m - 1) + 3], bound);
                for (int j = 0; j < m; j++) b.add(nb + 4 * j, nb[4 * j + 3], h2);
            }
            float rgb[3];
            b.result(rgb);
            out.insert(out.end(), rgb, rgb + 3);
        }
    } else if (!strcmp(mode, "mean")) {
        const size_t groups = (size_t)in.at(0);
        size_t at = 1;
        for (size_t gi = 0; gi < groups; gi++) {
            const int64_t count = (int64_t)in.at(at);
            const float* col = in.data() + at + 1;
            at += 1 + 3 * (size_t)count;
            if (count < 1 || at > in.size()) return 2;
            std::vector<sdfk_color::Sum3> chunks;
            for (int64_t q = 0; q < sdfk_color::chunks_of(count); q++) {
                const int64_t base = q * sdfk_color::kChunk;
                const int len = (int)(count - base < sdfk_color::kChunk ? count - base : sdfk_color::kChunk);
                chunks.push_back(sdfk_color::chunk_sum(col, len, [&](int t) { return base + t; }));
            }
            float rgb[3];
            sdfk_color::group_mean(count, [&](int64_t q) { return chunks[(size_t)q].v; }, rgb);
            out.insert(out.end(), rgb, rgb + 3);
        }
        if (at != in.size()) return 2;
    } else
        return 2;
    write_all(argv[3], out);
    printf("points_color_host %s ok\n", mode);
    return 0;
}
