// points_knn_host.cpp -- sdfkit_amd/csrc/points_knn.h built for the host (g++ -ffp-contract=off): the bounded candidate lists, the
// in-place heap sort, the radius predicate and the stopping rule as the kernels of lib_points_knn.hip run them, driven by
// tests/test_points_knn.py, which compares every answer with numpy.
//
//   points_knn_host list   IN OUT   IN: u64 kind (0 heap, 1 sorted<8>), u64 k, u64 m, m keys (offered in that order)
//                                   OUT: u64 count, then k keys (at(0..k-1) after finish)
//   points_knn_host sort   IN OUT   IN: u64 m, m keys -> OUT: the m keys ascending (heap_make + heap_sort)
//   points_knn_host radius IN OUT   IN: u32 m, m pairs (bits(r), bits(d2)) -> OUT: m x (u32 bits(radius_d2_bound(r)), u32 within)
//   points_knn_host stop   IN OUT   IN: u32 m, m x (bits(lb2), bits(worst d2), bits(bound)) -> OUT: m x u32 walk_done
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/points_knn.h"

using namespace sdfk_knn;

struct VecStore {
    std::vector<uint64_t> v;
    uint64_t get(int i) const { return v.at((size_t)i); }
    void set(int i, uint64_t key) { v.at((size_t)i) = key; }
};

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

template <class L>
static void run_list(L& list, int k, const uint64_t* keys, size_t m, std::vector<uint64_t>& out)
{
    list.init(k);
    for (size_t i = 0; i < m; i++)
        if (keys[i] < list.worst()) list.insert(keys[i]);   // (the kernels' test; the radius bound is applied before it)
    list.finish();
    out.push_back((uint64_t)list.count());
    for (int i = 0; i < k; i++) out.push_back(list.at(i));
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const char* mode = argv[1];
    if (!strcmp(mode, "list")) {
        const auto in = read_all<uint64_t>(argv[2]);
        std::vector<uint64_t> out;
        const int k = (int)in.at(1);
        const size_t m = (size_t)in.at(2);
        if (in.size() != 3 + m || k < 1 || k > kMaxK) return 2;
        if (in[0] == 0) {
            HeapList<VecStore> list;
            list.s.v.assign((size_t)k, ~0ull);   // (a touch beyond slot k - 1 throws)
            run_list(list, k, in.data() + 3, m, out);
        } else {
            if (k > 8) return 2;
            SortedList<8> list;
            run_list(list, k, in.data() + 3, m, out);
        }
        write_all(argv[3], out);
    } else if (!strcmp(mode, "sort")) {
        const auto in = read_all<uint64_t>(argv[2]);
        VecStore s;
        s.v.assign(in.begin() + 1, in.end());
        if (s.v.size() != in.at(0)) return 2;
        heap_make(s, (int)s.v.size());
        heap_sort(s, (int)s.v.size());
        write_all(argv[3], s.v);
    } else if (!strcmp(mode, "radius")) {
        const auto in = read_all<uint32_t>(argv[2]);
        std::vector<uint32_t> out;
        for (uint32_t i = 0; i < in.at(0); i++) {
            const float r = bits_f32(in.at(1 + 2 * i)), d2 = bits_f32(in.at(2 + 2 * i));
            if (!radius_is_valid(r)) { out.push_back(0xffffffffu); out.push_back(2); continue; }
            const float b = radius_d2_bound(r);
            out.push_back(f32_bits(b));
            out.push_back(within(d2, b) ? 1u : 0u);
        }
        write_all(argv[3], out);
    } else if (!strcmp(mode, "stop")) {
        const auto in = read_all<uint32_t>(argv[2]);
        std::vector<uint32_t> out;
        for (uint32_t i = 0; i < in.at(0); i++)
            out.push_back(walk_done(bits_f32(in.at(1 + 3 * i)), (uint64_t)in.at(2 + 3 * i) << 32 | 7u, bits_f32(in.at(3 + 3 * i))) ? 1u : 0u);
        write_all(argv[3], out);
    } else
        return 2;
    printf("points_knn_host %s ok\n", mode);
    return 0;
}
