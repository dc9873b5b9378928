// points_cluster_host.cpp -- sdfkit_amd/csrc/points_cluster.h built for the host (g++ -ffp-contract=off): the within predicate on
// packed keys, the saturating count and the core rule, the hook of an edge and its "changed" test, the root test, the border
// point's choice, the keep rule of select and the argument checks as the kernels of lib_points_cluster.hip run them, driven by
// tests/test_points_cluster_model.py, which compares every answer with the numpy model (tests/points_cluster_model.py).
//
//   points_cluster_host within IN OUT   IN: f32 radius, then d2 values          OUT: i64 per d2: reaches(pack_key(d2, its position), bound)
//   points_cluster_host core IN OUT     IN: i32 pairs (count, min_points)       OUT: i64 2 per pair: is_core, count_add(count)
//   points_cluster_host hook IN OUT     IN: i32 quadruples (pi, pj, old, i)     OUT: i64 6 per case: hooked, at, offered, changes(old),
//                                                                                    is_root(i, pi, core = true), is_root(i, pi, false)
//   points_cluster_host border IN OUT   IN: u64 cases, per case: bound_key, m, then m x (key, candidate is core)
//                                                                               OUT: i64 per case: border_source of the fold from kKeyInf
//   points_cluster_host select IN OUT   IN: i64 n_clusters, keep bytes (one i64 each, n_clusters of them; none when < 1), then labels
//                                                                               OUT: i64 per label: keeps
//   points_cluster_host args IN OUT     IN: f64 cases of 7: has_set, radius, min_points, has_set, has_labels, has_keep, n_clusters
//                                                                               OUT: i64 3 per case: check_cluster_args, check_select_args, max_rounds(n_clusters)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/points_cluster.h"

using namespace sdfk_cluster;
using namespace sdfk_knn;

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
    std::vector<int64_t> out;
    if (!strcmp(mode, "within")) {
        const auto in = read_all<float>(argv[2]);
        const uint64_t bound = bound_key_of(in.at(0));
        for (size_t i = 1; i < in.size(); i++) out.push_back(reaches(pack_key(in[i], (int32_t)(i - 1)), bound) ? 1 : 0);
        // the index plays no part: the greatest one is within wherever the least is
        for (size_t i = 1; i < in.size(); i++)
            if (reaches(pack_key(in[i], -1), bound) != reaches(pack_key(in[i], 0), bound)) return 3;
    } else if (!strcmp(mode, "core")) {
        const auto in = read_all<int32_t>(argv[2]);
        if (in.size() % 2) return 2;
        for (size_t c = 0; c < in.size(); c += 2) {
            out.push_back(is_core(in[c], in[c + 1]) ? 1 : 0);
            out.push_back(count_add(in[c]));
        }
    } else if (!strcmp(mode, "hook")) {
        const auto in = read_all<int32_t>(argv[2]);
        if (in.size() % 4) return 2;
        for (size_t c = 0; c < in.size(); c += 4) {
            int32_t at = -1, offered = -1;
            const bool hooked = hook_edge(in[c], in[c + 1], &at, &offered);
            out.insert(out.end(), {hooked ? 1 : 0, at, offered, hooked && hook_changes(in[c + 2], offered) ? 1 : 0, is_root(in[c + 3], in[c], true) ? 1 : 0,
                                   is_root(in[c + 3], in[c], false) ? 1 : 0});
        }
    } else if (!strcmp(mode, "border")) {
        const auto in = read_all<uint64_t>(argv[2]);
        size_t at = 1;
        for (uint64_t c = 0; c < in.at(0); c++) {
            const uint64_t bound = in.at(at), m = in.at(at + 1);
            at += 2;
            uint64_t best = kKeyInf;
            for (uint64_t j = 0; j < m; j++, at += 2) best = border_take(best, in.at(at), bound, in.at(at + 1) != 0);
            out.push_back(border_source(best));
        }
        if (at != in.size()) return 2;
    } else if (!strcmp(mode, "select")) {
        const auto in = read_all<int64_t>(argv[2]);
        const int64_t C = in.at(0);
        std::vector<uint8_t> keep;
        size_t at = 1;
        for (int64_t c = 0; c < C; c++) keep.push_back((uint8_t)in.at(at++));
        for (; at < in.size(); at++) out.push_back(keeps((int32_t)in[at], C, keep.data()) ? 1 : 0);   // (keep.data() may be null: never read then)
    } else if (!strcmp(mode, "args")) {
        const auto in = read_all<double>(argv[2]);
        if (in.size() % 7) return 2;
        for (size_t c = 0; c < in.size(); c += 7) {
            out.push_back(check_cluster_args(in[c] != 0, (float)in[c + 1], (int32_t)in[c + 2]));
            out.push_back(check_select_args(in[c + 3] != 0, in[c + 4] != 0, in[c + 5] != 0, (int64_t)in[c + 6]));
            out.push_back(max_rounds((int64_t)in[c + 6]));
        }
    } else
        return 2;
    write_all(argv[3], out);
    printf("points_cluster_host %s ok\n", mode);
    return 0;
}
