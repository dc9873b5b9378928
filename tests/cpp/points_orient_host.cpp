// points_orient_host.cpp -- sdfkit_amd/csrc/points_orient.h built for the host (g++ -ffp-contract=off): validity, the seed's order
// and sign, one point's choice from its row and the level rule as the kernels of lib_orient.hip run them, driven by
// tests/test_orient_model.py, which compares every answer with tests/orient_model.py.
//
//   points_orient_host choose IN OUT   IN (f32): cases, then per case: found, round, level, n_i (3), 64 x (n_j (3), stamp, sign)
//                                      OUT (i32): per case accepted (0 / 1), sign (+-1)
//   points_orient_host seed   IN OUT   IN (f32): cases, then per case a normal (3)
//                                      OUT (i32): per case valid (0 / 1), the seed's sign, the bits of the flipped first component
//   points_orient_host pick   IN OUT   IN (f32): lists, length, then per list `length` x (z, candidate 0 / 1)
//                                      OUT (i32): per list the index of the greatest seed key among the candidates, -1 without one
//   points_orient_host level  IN OUT   IN (i32): pairs (level, count) -> OUT (i32): the next level
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/points_orient.h"

using namespace sdfk_orient;

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

static void write_all(const char* path, const std::vector<int32_t>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(int32_t), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const char* mode = argv[1];
    std::vector<int32_t> out;
    if (!strcmp(mode, "choose")) {
        const auto in = read_all<float>(argv[2]);
        const size_t cases = (size_t)in.at(0), stride = 6 + 5 * 64;
        if (in.size() != 1 + cases * stride) return 2;
        for (size_t c = 0; c < cases; c++) {
            const float* r = in.data() + 1 + c * stride;
            const int found = (int)r[0], round = (int)r[1], level = (int)r[2];
            const float* ni = r + 3;
            Choice ch;
            for (int j = 0; j < found; j++) {
                const float* e = r + 6 + 5 * j;
                if (is_source((int32_t)e[3], round, e)) ch.offer(ni, e, (int)e[4]);
            }
            out.push_back(ch.accepted(level) ? 1 : 0);
            out.push_back(ch.sign());
        }
    } else if (!strcmp(mode, "seed")) {
        const auto in = read_all<float>(argv[2]);
        const size_t cases = (size_t)in.at(0);
        if (in.size() != 1 + cases * 3) return 2;
        for (size_t c = 0; c < cases; c++) {
            const float* n = in.data() + 1 + 3 * c;
            out.push_back(valid(n) ? 1 : 0);
            out.push_back(seed_sign(n));
            out.push_back((int32_t)sdfk_knn::f32_bits(flipped(n[0])));
        }
    } else if (!strcmp(mode, "pick")) {
        const auto in = read_all<float>(argv[2]);
        const size_t lists = (size_t)in.at(0), len = (size_t)in.at(1);
        if (in.size() != 2 + lists * len * 2) return 2;
        for (size_t l = 0; l < lists; l++) {
            const float* r = in.data() + 2 + l * len * 2;
            uint64_t best = 0;
            for (size_t i = len; i-- > 0;) {   // (backwards: the maximum does not depend on the order of arrival)
                if (r[2 * i + 1] == 0.0f) continue;
                const uint64_t key = seed_key(r[2 * i], (int32_t)i);
                best = key > best ? key : best;
            }
            out.push_back(best ? seed_index(best) : -1);
        }
    } else if (!strcmp(mode, "level")) {
        const auto in = read_all<int32_t>(argv[2]);
        for (size_t i = 0; i + 1 < in.size(); i += 2) out.push_back(next_level(in[i], (unsigned)in[i + 1]));
    } else
        return 2;
    write_all(argv[3], out);
    printf("points_orient_host %s ok\n", mode);
    return 0;
}
