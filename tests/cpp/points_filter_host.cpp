// points_filter_host.cpp -- sdfkit_amd/csrc/points_filter.h built for the host (g++ -ffp-contract=off): the voxel key and its range
// refusal, the chunked centroid sum and the outlier threshold / keep rule as the kernels of lib_points_filter.hip run them, driven by
// tests/test_points_filter_model.py, which compares every answer with the numpy model (tests/points_filter_model.py).
//
//   points_filter_host key IN OUT   IN: f32 size, origin (3), n, then n x 3 coordinates
//                                   OUT: i64 status (0 accepted, 1 size, 2 origin, 3 span), pass mask, then n packed keys
//   points_filter_host sum IN OUT   IN: f32 cases, per case: count, then count x 3 coordinates (one voxel's members in order)
//                                   OUT: f32 3 per case: the centroid
//   points_filter_host thr IN OUT   IN: f64 cases, per case: sum, sqsum, c, std_ratio, sum_rest, found
//                                   OUT: f64 5 per case: mu, sigma, thr, mean, kept (mu from a first call with sqsum = 0, as the kernels)
//   points_filter_host ratio IN OUT IN: f32 ratios
//                                   OUT: i64 per ratio: 1 accepted, 0 refused (ratio_is_valid, what sdfk_points_outliers asks first)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/points_filter.h"

using namespace sdfk_filter;

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
    if (!strcmp(mode, "key")) {
        const auto in = read_all<float>(argv[2]);
        const float size = in.at(0), origin[3] = {in.at(1), in.at(2), in.at(3)};
        const size_t n = (size_t)in.at(4);
        if (in.size() != 5 + 3 * n || n < 1) return 2;
        const float* p = in.data() + 5;
        std::vector<int64_t> out;
        if (!size_is_valid(size)) out = {1, 0};
        else if (!origin_is_valid(origin)) out = {2, 0};
        else {
            // the library takes the extreme voxels from the set's box: the least and greatest coordinate of each axis
            Lattice L{};
            L.size = size;
            int bits[3];
            bool ok = true;
            for (int a = 0; a < 3; a++) {
                float lo = p[a], hi = p[a];
                for (size_t i = 1; i < n; i++) { lo = p[3 * i + a] < lo ? p[3 * i + a] : lo; hi = p[3 * i + a] > hi ? p[3 * i + a] : hi; }
                L.origin[a] = origin[a];
                const double kmin = voxel_of(lo, origin[a], size), kmax = voxel_of(hi, origin[a], size);
                ok = ok && span_is_valid(kmin, kmax);
                if (!ok) break;
                L.kmin[a] = kmin;
                bits[a] = span_bits(kmin, kmax);
            }
            if (!ok) out = {3, 0};
            else {
                out = {0, (int64_t)digit_mask(bits)};
                for (size_t i = 0; i < n; i++) out.push_back((int64_t)voxel_key(L, p[3 * i], p[3 * i + 1], p[3 * i + 2]));
            }
        }
        write_all(argv[3], out);
    } else if (!strcmp(mode, "sum")) {
        const auto in = read_all<float>(argv[2]);
        std::vector<float> out;
        size_t at = 1;
        for (size_t c = 0; c < (size_t)in.at(0); c++) {
            const int64_t count = (int64_t)in.at(at++);
            Sum3 total;
            for (int64_t q = 0; q < chunks_of(count); q++) {
                Sum3 chunk;
                for (int64_t t = q * kChunk; t < count && t < (q + 1) * kChunk; t++) chunk.add_point(in.at(at + 3 * t), in.at(at + 3 * t + 1), in.at(at + 3 * t + 2));
                total.add_sum(chunk.v);
            }
            at += 3 * (size_t)count;
            for (int a = 0; a < 3; a++) out.push_back(centroid_of(total.v[a], count));
        }
        if (at != in.size()) return 2;
        write_all(argv[3], out);
    } else if (!strcmp(mode, "thr")) {
        const auto in = read_all<double>(argv[2]);
        std::vector<double> out;
        for (size_t c = 0; c < (size_t)in.at(0); c++) {
            const double* v = &in.at(1 + 6 * c);
            (void)in.at(6 + 6 * c);
            const Threshold T = threshold_of(v[0], v[1], v[2], (float)v[3]);
            const double mean = row_mean(v[4], (int)v[5]);
            out.insert(out.end(), {T.mu, T.sigma, T.thr, mean, is_kept(mean, T.thr) ? 1.0 : 0.0});
            if (threshold_of(v[0], 0.0, v[2], 0.0f).mu != T.mu && T.mu == T.mu) return 3;   // (the mean does not depend on the second sum)
        }
        write_all(argv[3], out);
    } else if (!strcmp(mode, "ratio")) {
        const auto in = read_all<float>(argv[2]);
        std::vector<int64_t> out;
        for (float r : in) out.push_back(ratio_is_valid(r) ? 1 : 0);
        write_all(argv[3], out);
    } else
        return 2;
    printf("points_filter_host %s ok\n", mode);
    return 0;
}
