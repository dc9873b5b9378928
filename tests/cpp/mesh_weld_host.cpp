// mesh_weld_host.cpp -- runs the decisions of sdfkit_amd/csrc/trimesh_weld.h (the functions the kernels of lib_trimesh_weld.hip
// call) on the host, in the order of the kernels but one item at a time, for tests/test_mesh_weld_host.py to compare with the
// numpy model.  usage: mesh_weld_host MODE in out
//   weld      in: int64 nv, nt, flags; f32 tolerance, pad; uint32 P[3 nv] (the bits of the positions); int32 T[3 nt]
//             out (int64): status (0; 1: refused), passes, groups, kv, kt, vertex_map[nv], vertex_index[kv], triangle_index[kt],
//                          triangles[3 kt]
//   keys      in: uint32 (p, q) position pairs, 6 each      out (uint64): first key of p, second key of p, exact_same(p, q)
//   mask      in: uint64 diffs                              out: uint32 (mask, passes) pairs
//   ordered   in: uint32 bits                               out: uint32 (ordered, back) pairs
//   keep      in: int32 (a, b, c, v, rep_v, used, flags)    out: int32 (keeps_triangle, keeps_vertex, flags_are_valid, map_of(used, 5)) per row
//   lattice   in: f32 tolerance, lo[3], hi[3]; then uint32 P[3 n]
//             out (int64): valid, tolerance_is_valid, mask, then the n keys (nothing after the first three when not valid)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sdfkit_amd/csrc/trimesh_weld.h"

using namespace sdfk_trimesh_wld;

struct Rec {
    uint64_t key;
    uint32_t index;
};

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

template <class T>
static void put(FILE* f, const std::vector<T>& v)
{
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

// the passes of `mask`, least byte first, each a stable counting of one byte: what device_sort.h does
static void radix(std::vector<Rec>& r, unsigned mask)
{
    for (int d = 0; d < 8; d++)
        if (mask >> d & 1u)
            std::stable_sort(r.begin(), r.end(), [d](const Rec& a, const Rec& b) { return (a.key >> (8 * d) & 255u) < (b.key >> (8 * d) & 255u); });
}

static int weld(const std::vector<char>& in, FILE* out)
{
    int64_t head[3];
    float tol[2];
    memcpy(head, in.data(), sizeof head);
    memcpy(tol, in.data() + sizeof head, sizeof tol);
    const int64_t nv = head[0], nt = head[1];
    const int32_t flags = (int32_t)head[2];
    const uint32_t* P = (const uint32_t*)(in.data() + sizeof head + sizeof tol);
    const int32_t* T = (const int32_t*)(P + 3 * nv);
    const std::vector<int64_t> refused = {1};
    if (!tolerance_is_valid(tol[0]) || !flags_are_valid(flags)) { put(out, refused); return 0; }
    const bool exact = tol[0] == 0.0f;
    Lattice L{};
    unsigned lattice_mask = 0xffu;
    if (!exact) {   // k_tw_bounds
        uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0, 0, 0};
        for (int64_t v = 0; v < nv; v++)
            for (int a = 0; a < 3; a++) {
                lo[a] = std::min(lo[a], ordered_bits(P[3 * v + a]));
                hi[a] = std::max(hi[a], ordered_bits(P[3 * v + a]));
            }
        float flo[3], fhi[3];
        for (int a = 0; a < 3; a++) { flo[a] = float_of(unordered_bits(lo[a])); fhi[a] = float_of(unordered_bits(hi[a])); }
        if (!lattice_of(tol[0], flo, fhi, &L, &lattice_mask)) { put(out, refused); return 0; }
    }
    // k_tw_keys
    std::vector<Rec> rec(nv);
    uint64_t diff[2] = {0, 0};
    for (int64_t v = 0; v < nv; v++) {
        const uint64_t key = exact ? exact_key_first(P + 3 * v) : lattice_key(L, P + 3 * v);
        rec[v] = Rec{key, (uint32_t)v};
        diff[0] |= key_diff(key, exact ? exact_key_first(P) : lattice_key(L, P));
        if (exact) diff[1] |= key_diff(exact_key_second(P + 3 * v), exact_key_second(P));
    }
    int passes = 0;
    {
        const unsigned mask = pass_mask(diff[0]) & lattice_mask;
        passes += passes_of(mask);
        radix(rec, mask);
    }
    if (exact) {
        const unsigned mask = pass_mask(diff[1]);
        if (mask) {
            for (Rec& r : rec) r.key = exact_key_second(P + 3 * r.index);   // k_tw_rekey
            passes += passes_of(mask);
            radix(rec, mask);
        }
    }
    // k_tw_heads, the scan, k_tw_first, k_tw_rep
    std::vector<uint32_t> scanned(nv + 1, 0);
    for (int64_t j = 0; j < nv; j++) {
        const bool same = j > 0 && (exact ? exact_same(P + 3 * rec[j].index, P + 3 * rec[j - 1].index) : rec[j].key == rec[j - 1].key);
        scanned[j + 1] = scanned[j] + (is_head(j, same) ? 1u : 0u);
    }
    const int64_t groups = scanned[nv];
    std::vector<int32_t> group_first(nv, -1), rep(nv, -1);
    for (int64_t j = 0; j < nv; j++)
        if (scanned[j + 1] != scanned[j]) group_first[scanned[j]] = (int32_t)rec[j].index;
    for (int64_t j = 0; j < nv; j++) rep[rec[j].index] = group_first[group_of(scanned[j], scanned[j + 1] != scanned[j])];
    // k_tw_tri_flags, k_tw_vert_flags, the scans
    std::vector<uint8_t> used(nv, 0);
    std::vector<int64_t> tnew(nt + 1, 0), vnew(nv + 1, 0);
    for (int64_t t = 0; t < nt; t++) {
        const int32_t a = rep[T[3 * t]], b = rep[T[3 * t + 1]], c = rep[T[3 * t + 2]];
        const bool keep = keeps_triangle(a, b, c, flags);
        tnew[t + 1] = tnew[t] + (keep ? 1 : 0);
        if (keep) used[a] = used[b] = used[c] = 1;
    }
    for (int64_t v = 0; v < nv; v++) vnew[v + 1] = vnew[v] + (keeps_vertex((int32_t)v, rep[v], used[v] != 0, flags) ? 1 : 0);
    // k_tw_vertices, k_tw_triangles
    std::vector<int64_t> vmap(nv), vi, ti, tr;
    for (int64_t v = 0; v < nv; v++) {
        const int64_t r = rep[v];
        const bool kept = vnew[r + 1] != vnew[r];
        vmap[v] = map_of(kept, (uint32_t)vnew[r]);
        if (r == v && kept) vi.push_back(v);
    }
    for (int64_t t = 0; t < nt; t++)
        if (tnew[t + 1] != tnew[t]) {
            ti.push_back(t);
            for (int k = 0; k < 3; k++) tr.push_back(vnew[rep[T[3 * t + k]]]);
        }
    const std::vector<int64_t> first = {0, passes, groups, (int64_t)vi.size(), (int64_t)ti.size()};
    put(out, first); put(out, vmap); put(out, vi); put(out, ti); put(out, tr);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 1;
    const std::string mode = argv[1];
    const std::vector<char> in = slurp(argv[2]);
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 1;
    int rc = 0;
    if (mode == "weld") {
        rc = weld(in, out);
    } else if (mode == "keys") {
        const uint32_t* p = (const uint32_t*)in.data();
        for (size_t i = 0; i + 5 < in.size() / 4; i += 6) {
            const uint64_t o[3] = {exact_key_first(p + i), exact_key_second(p + i), exact_same(p + i, p + i + 3) ? 1u : 0u};
            fwrite(o, 8, 3, out);
        }
    } else if (mode == "mask") {
        const uint64_t* p = (const uint64_t*)in.data();
        for (size_t i = 0; i < in.size() / 8; i++) {
            const uint32_t o[2] = {pass_mask(p[i]), (uint32_t)passes_of(pass_mask(p[i]))};
            fwrite(o, 4, 2, out);
        }
    } else if (mode == "ordered") {
        const uint32_t* p = (const uint32_t*)in.data();
        for (size_t i = 0; i < in.size() / 4; i++) {
            const uint32_t o[2] = {ordered_bits(p[i]), unordered_bits(ordered_bits(p[i]))};
            fwrite(o, 4, 2, out);
        }
    } else if (mode == "keep") {
        const int32_t* p = (const int32_t*)in.data();
        for (size_t i = 0; i + 6 < in.size() / 4; i += 7) {
            const int32_t o[4] = {keeps_triangle(p[i], p[i + 1], p[i + 2], p[i + 6]), keeps_vertex(p[i + 3], p[i + 4], p[i + 5] != 0, p[i + 6]),
                                  flags_are_valid(p[i + 6]), map_of(p[i + 5] != 0, 5u)};
            fwrite(o, 4, 4, out);
        }
    } else if (mode == "lattice") {
        float h[7];
        memcpy(h, in.data(), sizeof h);
        const uint32_t* P = (const uint32_t*)(in.data() + sizeof h);
        const size_t n = (in.size() - sizeof h) / 12;
        Lattice L{};
        unsigned mask = 0;
        const bool tol_ok = tolerance_is_valid(h[0]);
        const bool ok = tol_ok && h[0] > 0.0f && lattice_of(h[0], h + 1, h + 4, &L, &mask);
        std::vector<int64_t> o = {ok ? 1 : 0, tol_ok ? 1 : 0, (int64_t)mask};
        if (ok)
            for (size_t i = 0; i < n; i++) o.push_back((int64_t)lattice_key(L, P + 3 * i));
        put(out, o);
    } else {
        rc = 1;
    }
    fclose(out);
    if (rc == 0) printf("mesh weld ok\n");
    return rc;
}
