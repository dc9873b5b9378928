// mesh_smooth_host.cpp -- runs the arithmetic and the decisions of sdfkit_amd/csrc/trimesh_adjacency.h (the functions the kernels
// of lib_trimesh_smooth.hip call) on the host, in the order of the kernels but one item at a time, for
// tests/test_mesh_smooth_host.py to compare with the numpy model.  usage: mesh_smooth_host in out
//   in:  int64 nv, nt, iterations, flags (1: pin the boundary, 2: flip the normals); float lambda, mu; int32 T[3 nt]; float V[3 nv]
//   out (uint32 words): the two sort masks; E, nbr_start[nv + 1], nbr[E], boundary[nv]; IE, inc_start[nv + 1], inc[IE];
//        then the bits of: smoothed[3 nv], the normals of V [3 nv], the normals of the smoothed positions (flipped if asked) [3 nv]
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/trimesh_adjacency.h"

using namespace sdfk_trimesh_adj;

struct R { uint64_t key; uint32_t index; };

static std::vector<char> slurp(const char* path)
{
    std::vector<char> b;
    FILE* f = fopen(path, "rb");
    if (!f) return b;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

static void put(FILE* f, const std::vector<uint32_t>& v)
{
    if (!v.empty()) fwrite(v.data(), 4, v.size(), f);
}

// k_ta_heads + scan, k_ta_entries, k_ta_degree + scan over the sorted records; false: the degrees do not add up
static bool rows(const std::vector<R>& s, int64_t nv, int shift, std::vector<uint32_t>& start, std::vector<uint32_t>& list, std::vector<uint32_t>* boundary)
{
    const int64_t n = (int64_t)s.size();
    std::vector<uint32_t> place(n + 1, 0), begin(nv, 0xFFFFFFFFu), degree(nv + 1, 0);
    for (int64_t j = 0; j < n; j++)
        place[j + 1] = place[j] + ((shift == 0 ? record_vertex(s[j].key, 0) < nv : entry_head(s[j].key, j > 0, j > 0 ? s[j - 1].key : 0, nv, shift)) ? 1u : 0u);
    list.assign(place[n], 0xFFFFFFFFu);
    if (boundary) boundary->assign(nv, 0);
    for (int64_t j = 0; j < n; j++) {
        const uint64_t key = s[j].key;
        const int64_t v = record_vertex(key, shift);
        if (v >= nv) continue;
        const bool has_prev = j > 0, has_next = j + 1 < n;
        const uint64_t prev = has_prev ? s[j - 1].key : 0, next = has_next ? s[j + 1].key : 0;
        const bool entry = shift == 0 || entry_head(key, has_prev, prev, nv, shift);
        const uint32_t at = shift == 0 ? (uint32_t)j : place[j];
        if (entry) {
            if (at >= list.size()) return false;
            list[at] = shift == 0 ? s[j].index : (uint32_t)key;
        }
        if (vertex_first(key, has_prev, prev, nv, shift)) begin[v] = at;
        if (boundary && run_of_one(key, has_prev, prev, has_next, next)) { (*boundary)[v] = 1; (*boundary)[(uint32_t)key] = 1; }
    }
    for (int64_t j = 0; j < n; j++) {
        const uint64_t key = s[j].key;
        const int64_t v = record_vertex(key, shift);
        if (v >= nv) continue;
        const bool has_next = j + 1 < n;
        if (vertex_last(key, has_next, has_next ? s[j + 1].key : 0, nv, shift)) degree[v] = (shift == 0 ? (uint32_t)(j + 1) : place[j + 1]) - begin[v];
    }
    start.assign(nv + 1, 0);
    for (int64_t v = 0; v < nv; v++) start[v + 1] = start[v] + degree[v];
    return start[nv] == list.size();
}

// the sort of device_sort.h: stable, and only the bytes of the mask take part
static void sort_masked(std::vector<R>& rec, unsigned mask)
{
    uint64_t bits = 0;
    for (int d = 0; d < 8; d++)
        if (mask >> d & 1u) bits |= 0xFFull << (8 * d);
    std::stable_sort(rec.begin(), rec.end(), [bits](const R& a, const R& b) { return (a.key & bits) < (b.key & bits); });
}

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    const std::vector<char> in = slurp(argv[1]);
    int64_t head[4];
    float factors[2];
    if (in.size() < sizeof head + sizeof factors) return 1;
    memcpy(head, in.data(), sizeof head);
    memcpy(factors, in.data() + sizeof head, sizeof factors);
    const int64_t nv = head[0], nt = head[1], iterations = head[2], flags = head[3];
    const float lambda = factors[0], mu = factors[1];
    if (in.size() != sizeof head + sizeof factors + 12 * (size_t)nt + 12 * (size_t)nv) return 1;
    const int32_t* T = (const int32_t*)(in.data() + sizeof head + sizeof factors);
    const float* V = (const float*)(in.data() + sizeof head + sizeof factors + 12 * nt);
    if (too_many_triangles(nt)) return 2;

    std::vector<R> nrec, crec;
    for (int64_t t = 0; t < nt; t++) {
        const int32_t tri[3] = {T[3 * t], T[3 * t + 1], T[3 * t + 2]};
        const bool skip = index_degenerate(tri[0], tri[1], tri[2]);
        for (int j = 0; j < 6; j++) {
            int32_t from, to;
            directed_record(tri, j, &from, &to);
            nrec.push_back(R{skip ? nbr_skip_key(nv) : nbr_key(from, to), (uint32_t)t});
        }
        for (int k = 0; k < 3; k++) crec.push_back(R{skip ? corner_skip_key(nv) : (uint64_t)tri[k], (uint32_t)(3 * t + k)});
    }
    sort_masked(nrec, nbr_digit_mask(nv));
    sort_masked(crec, corner_digit_mask(nv));
    std::vector<uint32_t> nbr_start, nbr, boundary, inc_start, inc;
    if (!rows(nrec, nv, 32, nbr_start, nbr, &boundary)) return 3;
    if (!rows(crec, nv, 0, inc_start, inc, nullptr)) return 3;

    // the steps: ping-pong, every step reads the buffer of the one before
    std::vector<float> a(V, V + 3 * nv), b(3 * nv);
    const int64_t steps = smooth_steps((int32_t)iterations, mu);
    for (int64_t i = 0; i < steps; i++) {
        for (int64_t v = 0; v < nv; v++)
            smooth_vertex(a.data(), nbr.data(), nbr_start[v], nbr_start[v + 1], (flags & 1) && boundary[v] != 0, smooth_factor(i, lambda, mu), v, &b[3 * v]);
        a.swap(b);
    }
    std::vector<float> n0(3 * nv), n1(3 * nv);
    for (int64_t v = 0; v < nv; v++) {
        vertex_normal(V, T, inc.data(), inc_start[v], inc_start[v + 1], false, &n0[3 * v]);
        vertex_normal(a.data(), T, inc.data(), inc_start[v], inc_start[v + 1], (flags & 2) != 0, &n1[3 * v]);
    }

    FILE* out = fopen(argv[2], "wb");
    if (!out) return 1;
    put(out, {nbr_digit_mask(nv), corner_digit_mask(nv), (uint32_t)nbr.size()});
    put(out, nbr_start); put(out, nbr); put(out, boundary);
    put(out, {(uint32_t)inc.size()});
    put(out, inc_start); put(out, inc);
    fwrite(a.data(), 4, a.size(), out); fwrite(n0.data(), 4, n0.size(), out); fwrite(n1.data(), 4, n1.size(), out);
    fclose(out);
    printf("mesh smooth ok\n");
    return 0;
}
