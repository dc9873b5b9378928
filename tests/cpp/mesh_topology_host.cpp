// mesh_topology_host.cpp -- runs the decisions of sdfkit_amd/csrc/trimesh_topology.h (the functions the kernels of
// lib_trimesh_topology.hip call) on the host, in the order of the kernels but one item at a time, for
// tests/test_mesh_topology_host.py to compare with the numpy model.  usage: mesh_topology_host MODE in out
//   topology  in: int64 nv, nt, C_keep; int32 T[3 nt]; int64 w[nt]; uint8 keep[C_keep]
//             out (int64): C, rounds, shortcuts, vertex[nv], triangle[nt], rows[8 C], census[8], kv, kt, vertex_index[kv],
//                          triangle_index[kt], triangles[3 kt]
//   class     in: uint32 (m, f) pairs                      out: uint32 class bits, uint64 packed
//   mask      in: int64 nv                                 out: uint32 (bytes, mask) pairs
//   derive    in: int64 rows[8 n], then int64 min_triangles, total; double fraction (the last 24 bytes)
//             out (int64): per row euler, watertight, oriented, keep_by_size; then n x n larger_than
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sdfkit_amd/csrc/trimesh_topology.h"

using namespace sdfk_trimesh_topo;

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

static int topology(const std::vector<char>& in, FILE* out)
{
    int64_t head[3];
    memcpy(head, in.data(), sizeof head);
    const int64_t nv = head[0], nt = head[1], ck = head[2];
    const int32_t* T = (const int32_t*)(in.data() + sizeof head);
    const int64_t* w = (const int64_t*)(in.data() + sizeof head + 12 * nt);
    const uint8_t* keep = (const uint8_t*)(in.data() + sizeof head + 12 * nt + 8 * nt);
    // labels: k_tt_init, k_tt_ref, then hook rounds and shortcut launches (here one item after the other: every read is fresh)
    std::vector<int32_t> parent(nv);
    std::vector<uint8_t> referenced(nv, 0);
    for (int64_t v = 0; v < nv; v++) parent[v] = (int32_t)v;
    for (int64_t t = 0; t < nt; t++)
        if (!index_degenerate(T[3 * t], T[3 * t + 1], T[3 * t + 2]))
            for (int k = 0; k < 3; k++) referenced[T[3 * t + k]] = 1;
    int64_t rounds = 0, shortcuts = 0;
    for (;;) {
        if (rounds >= max_rounds(nv)) return 2;
        rounds++;
        int64_t changed = 0;
        for (int64_t t = 0; t < nt; t++) {
            if (index_degenerate(T[3 * t], T[3 * t + 1], T[3 * t + 2])) continue;
            const int32_t p[3] = {parent[T[3 * t]], parent[T[3 * t + 1]], parent[T[3 * t + 2]]};
            const int32_t m = hook_target(p[0], p[1], p[2]);
            for (int k = 0; k < 3; k++) {
                if (p[k] == m) continue;
                const int32_t old = parent[p[k]];   // atomicMin
                if (m < old) parent[p[k]] = m;
                if (hook_changes(old, m)) changed++;
            }
        }
        if (!changed) break;
        for (;;) {
            int64_t moved = 0;
            for (int64_t v = 0; v < nv; v++) {
                const int32_t p = parent[v], gp = parent[p];
                if (gp < p) { parent[v] = gp; moved++; }
            }
            if (!moved) break;
            shortcuts++;
        }
    }
    std::vector<int64_t> number(nv + 1, 0);
    for (int64_t v = 0; v < nv; v++) number[v + 1] = number[v] + (is_root((int32_t)v, parent[v], referenced[v] != 0) ? 1 : 0);
    const int64_t C = number[nv];
    std::vector<int64_t> vertex(nv), triangle(nt);
    for (int64_t v = 0; v < nv; v++) vertex[v] = referenced[v] ? number[parent[v]] : -1;
    for (int64_t t = 0; t < nt; t++) triangle[t] = index_degenerate(T[3 * t], T[3 * t + 1], T[3 * t + 2]) ? -1 : vertex[T[3 * t]];
    // rows and census
    std::vector<int64_t> rows(8 * C, 0), census(8, 0);
    census[kCensusComponents] = C;
    struct R { uint64_t key; uint32_t fwd; };
    std::vector<R> rec;
    for (int64_t t = 0; t < nt; t++) {
        const int32_t tri[3] = {T[3 * t], T[3 * t + 1], T[3 * t + 2]};
        if (index_degenerate(tri[0], tri[1], tri[2])) { census[kCensusDegenerate]++; rec.insert(rec.end(), 3, R{kSkipKey, 0}); continue; }
        rows[8 * triangle[t] + kTriangles]++;
        rows[8 * triangle[t] + kAreaWeight] += w[t];
        for (int k = 0; k < 3; k++) {
            int32_t u, v;
            directed_edge(tri, k, &u, &v);
            if (edge_key(u, v) == kSkipKey) return 3;
            rec.push_back(R{edge_key(u, v), edge_forward(u, v) ? 1u : 0u});
        }
    }
    for (int64_t v = 0; v < nv; v++)
        if (vertex[v] >= 0) { rows[8 * vertex[v] + kVertices]++; census[kCensusVertices]++; }
    std::stable_sort(rec.begin(), rec.end(), [](const R& a, const R& b) { return a.key < b.key; });
    for (size_t j = 0; j < rec.size();) {
        size_t e = j;
        uint32_t f = 0;
        while (e < rec.size() && rec[e].key == rec[j].key) f += rec[e++].fwd;
        if (rec[j].key != kSkipKey) {
            const uint64_t packed = edge_packed(edge_class((uint32_t)(e - j), f));
            const int64_t c = vertex[edge_low_vertex(rec[j].key)];
            for (int k = 0; k < 5; k++) {
                rows[8 * c + kEdges + k] += (int64_t)packed_byte(packed, k);
                census[kCensusEdges + k] += (int64_t)packed_byte(packed, k);
            }
        }
        j = e;
    }
    // select
    std::vector<int64_t> vnew(nv + 1, 0), vi, ti, tr;
    if (ck == C) {
        for (int64_t v = 0; v < nv; v++) {
            const bool k = keeps((int32_t)vertex[v], keep);
            vnew[v + 1] = vnew[v] + (k ? 1 : 0);
            if (k) vi.push_back(v);
        }
        for (int64_t t = 0; t < nt; t++)
            if (keeps((int32_t)triangle[t], keep)) {
                ti.push_back(t);
                for (int k = 0; k < 3; k++) tr.push_back(vnew[T[3 * t + k]]);
            }
    }
    const std::vector<int64_t> first = {C, rounds, shortcuts}, counts = {(int64_t)vi.size(), (int64_t)ti.size()};
    put(out, first); put(out, vertex); put(out, triangle); put(out, rows); put(out, census); put(out, counts); put(out, vi); put(out, ti); put(out, tr);
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
    if (mode == "topology") {
        rc = topology(in, out);
    } else if (mode == "class") {
        const uint32_t* p = (const uint32_t*)in.data();
        for (size_t i = 0; i + 1 < in.size() / 4; i += 2) {
            const unsigned cls = edge_class(p[i], p[i + 1]);
            const uint64_t o[2] = {cls, edge_packed(cls)};
            fwrite(o, 8, 2, out);
        }
    } else if (mode == "mask") {
        const int64_t* p = (const int64_t*)in.data();
        for (size_t i = 0; i < in.size() / 8; i++) {
            const uint32_t o[2] = {(uint32_t)index_bytes(p[i]), key_digit_mask(p[i])};
            fwrite(o, 4, 2, out);
        }
    } else if (mode == "derive") {
        const size_t n = (in.size() - 24) / 64;
        const int64_t* rows = (const int64_t*)in.data();
        int64_t mt, total;
        double frac;
        memcpy(&mt, in.data() + 64 * n, 8); memcpy(&total, in.data() + 64 * n + 8, 8); memcpy(&frac, in.data() + 64 * n + 16, 8);
        for (size_t i = 0; i < n; i++) {
            const int64_t* r = rows + 8 * i;
            const int64_t o[4] = {euler_characteristic(r[kVertices], r[kEdges], r[kTriangles]), is_watertight(r), is_oriented(r),
                                  keep_by_size(r, mt, frac, total)};
            fwrite(o, 8, 4, out);
        }
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < n; j++) {
                const int64_t o = larger_than(rows + 8 * i, rows + 8 * j);
                fwrite(&o, 8, 1, out);
            }
    } else {
        rc = 1;
    }
    fclose(out);
    if (rc == 0) printf("mesh topology ok\n");
    return rc;
}
