// mesh_simplify_host.cpp -- runs the decisions and the arithmetic of sdfkit_amd/csrc/trimesh_simplify.h (the functions the kernels
// of lib_trimesh_simplify.hip call) on the host, in the order of the kernels but one item at a time, for
// tests/test_mesh_simplify_host.py to compare with the numpy model.  usage: mesh_simplify_host MODE in out
//   simplify  in: int64 nv, nt, flags, placement, has_colors; f32 cell, pad; uint32 P[3 nv] (the bits of the positions);
//                 int32 T[3 nt]; f32 colours[3 nv] when has_colors
//             out (int64): status (0; 1: refused), kv, kt, stats[6], vertex_map[nv], vertex_index[kv], triangle_index[kt],
//                          triangles[3 kt], the bits of positions[3 kv], the bits of colours[3 kv]
//   args      in: rows of (f32 cell, int32 placement, int32 flags)   out: int32 (cell_is_valid, placement_is_valid, flags_are_known,
//                                                                               flags_are_compatible) per row
//   triple    in: uint32 (a, b, c, groups) rows     out (uint64): lo, mid, hi, has_vertex_set, first key, second key, mask of the
//                                                                 first sort, mask of the second
//   run       in: int32 (set, first, run, flags) rows               out: int32 keeps_in_run per row
//   cell      in: f64 (p, k, cell) rows, cell an f32 value               out: int32 in_cell per row
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sdfkit_amd/csrc/trimesh_simplify.h"

using namespace sdfk_trimesh_simp;
namespace wld = sdfk_trimesh_wld;

struct Rec {
    uint64_t key;
    uint32_t index, pad;
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

struct Members {
    const uint32_t* order;
    uint32_t operator()(int64_t i) const { return order[i]; }
};

static int simplify(const std::vector<char>& in, FILE* out)
{
    int64_t head[5];
    float cellpad[2];
    memcpy(head, in.data(), sizeof head);
    memcpy(cellpad, in.data() + sizeof head, sizeof cellpad);
    const int64_t nv = head[0], nt = head[1];
    const int32_t flags = (int32_t)head[2], placement = (int32_t)head[3];
    const float cell = cellpad[0];
    const uint32_t* P = (const uint32_t*)(in.data() + sizeof head + sizeof cellpad);
    const int32_t* T = (const int32_t*)(P + 3 * nv);
    const float* col = head[4] ? (const float*)(T + 3 * nt) : nullptr;
    const float* pos = (const float*)P;
    const std::vector<int64_t> refused = {1};
    if (!cell_is_valid(cell) || !placement_is_valid(placement) || !flags_are_known(flags) || !flags_are_compatible(flags)) { put(out, refused); return 0; }
    // ---- trimesh_groups (lib_trimesh_weld.hip, lattice mode) ----
    wld::Lattice L{};
    unsigned lattice_mask = 0xffu;
    {
        uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0, 0, 0};
        for (int64_t v = 0; v < nv; v++)
            for (int a = 0; a < 3; a++) {
                lo[a] = std::min(lo[a], wld::ordered_bits(P[3 * v + a]));
                hi[a] = std::max(hi[a], wld::ordered_bits(P[3 * v + a]));
            }
        float flo[3], fhi[3];
        for (int a = 0; a < 3; a++) { flo[a] = wld::float_of(wld::unordered_bits(lo[a])); fhi[a] = wld::float_of(wld::unordered_bits(hi[a])); }
        if (!wld::lattice_of(cell, flo, fhi, &L, &lattice_mask)) { put(out, refused); return 0; }
    }
    std::vector<Rec> rec(nv);
    uint64_t diff = 0;
    for (int64_t v = 0; v < nv; v++) {
        const uint64_t key = wld::lattice_key(L, P + 3 * v);
        rec[v] = Rec{key, (uint32_t)v, 0u};
        diff |= wld::key_diff(key, wld::lattice_key(L, P));
    }
    int passes = 0;
    {
        const unsigned mask = wld::pass_mask(diff) & lattice_mask;
        passes += wld::passes_of(mask);
        radix(rec, mask);
    }
    std::vector<uint32_t> scanned(nv + 1, 0), order(nv), gstart(nv + 1, 0);
    for (int64_t j = 0; j < nv; j++) {
        const bool same = j > 0 && rec[j].key == rec[j - 1].key;
        scanned[j + 1] = scanned[j] + (wld::is_head(j, same) ? 1u : 0u);
        order[j] = rec[j].index;
    }
    const int64_t groups = scanned[nv];
    std::vector<int32_t> rep(nv, -1);
    for (int64_t j = 0; j < nv; j++) {   // k_ts_starts, k_tw_first, k_tw_rep
        if (scanned[j + 1] != scanned[j]) gstart[scanned[j]] = (uint32_t)j;
    }
    gstart[groups] = (uint32_t)nv;
    for (int64_t j = 0; j < nv; j++) rep[order[j]] = (int32_t)order[gstart[wld::group_of(scanned[j], scanned[j + 1] != scanned[j])]];
    // k_ts_is_rep and its scan: the group numbers by ascending representative
    std::vector<uint32_t> gnum(nv + 1, 0);
    for (int64_t v = 0; v < nv; v++) gnum[v + 1] = gnum[v] + (rep[v] == v ? 1u : 0u);
    // ---- triangles ----
    auto triple_of = [&](int64_t t) { return sorted_triple(gnum[rep[T[3 * t]]], gnum[rep[T[3 * t + 1]]], gnum[rep[T[3 * t + 2]]]); };
    std::vector<uint8_t> tflag(nt, 0), used(nv, 0);
    int64_t degenerate = 0;
    for (int64_t t = 0; t < nt; t++) degenerate += has_vertex_set(triple_of(t)) ? 0 : 1;   // k_ts_tri_keys' count
    if (!(flags & kKeepDuplicates)) {
        std::vector<Rec> tr(nt);
        for (int64_t t = 0; t < nt; t++) tr[t] = Rec{triple_key_first(triple_of(t)), (uint32_t)t, 0u};
        radix(tr, triple_mask_first(groups));
        for (Rec& r : tr) {   // k_ts_tri_rekey
            const Triple k = triple_of(r.index);
            r = Rec{triple_key_second(k), r.index, k.lo};
        }
        radix(tr, triple_mask_second(groups));
        std::vector<uint32_t> th(nt + 1, 0), tstart(nt + 1, 0);
        for (int64_t j = 0; j < nt; j++) {
            const bool same = j > 0 && same_set(tr[j].key, tr[j].pad, tr[j - 1].key, tr[j - 1].pad);
            th[j + 1] = th[j] + (wld::is_head(j, same) ? 1u : 0u);
        }
        for (int64_t j = 0; j < nt; j++)
            if (th[j + 1] != th[j]) tstart[th[j]] = (uint32_t)j;
        tstart[th[nt]] = (uint32_t)nt;
        for (int64_t j = 0; j < nt; j++) {   // k_ts_tri_runs
            const bool first = th[j + 1] != th[j];
            const uint32_t run = first ? tstart[th[j] + 1] - (uint32_t)j : 0u;
            tflag[tr[j].index] = keeps_in_run(tr[j].key != 0ull, first, run, flags) ? 1 : 0;
        }
    } else {
        for (int64_t t = 0; t < nt; t++) tflag[t] = index_degenerate(rep[T[3 * t]], rep[T[3 * t + 1]], rep[T[3 * t + 2]]) ? 0 : 1;
    }
    for (int64_t t = 0; t < nt; t++)
        if (tflag[t]) used[rep[T[3 * t]]] = used[rep[T[3 * t + 1]]] = used[rep[T[3 * t + 2]]] = 1;
    std::vector<int64_t> tnew(nt + 1, 0), vnew(nv + 1, 0);
    for (int64_t t = 0; t < nt; t++) tnew[t + 1] = tnew[t] + tflag[t];
    for (int64_t v = 0; v < nv; v++) vnew[v + 1] = vnew[v] + (keeps_group((int32_t)v, rep[v], used[v] != 0) ? 1 : 0);
    const int64_t kv = vnew[nv], kt = tnew[nt];
    // ---- the adjacency's corner lists (lib_trimesh_smooth.hip) ----
    std::vector<uint32_t> inc_start(nv + 1, 0), inc;
    {
        std::vector<std::vector<uint32_t>> of(nv);
        for (int64_t t = 0; t < nt; t++) {
            if (index_degenerate(T[3 * t], T[3 * t + 1], T[3 * t + 2])) continue;
            for (int k = 0; k < 3; k++) of[T[3 * t + k]].push_back((uint32_t)(3 * t + k));
        }
        for (int64_t v = 0; v < nv; v++) {
            inc_start[v + 1] = inc_start[v] + (uint32_t)of[v].size();
            inc.insert(inc.end(), of[v].begin(), of[v].end());
        }
        inc.push_back(0u);   // (never an empty array)
    }
    // ---- k_ts_place ----
    std::vector<int64_t> opos(3 * kv), ocol(3 * kv);
    int64_t fallbacks = 0;
    for (int64_t grp = 0; grp < groups; grp++) {
        const uint32_t begin = gstart[grp], end = gstart[grp + 1];
        const int64_t r = order[begin], o = vnew[r];
        if (vnew[r + 1] == o) continue;
        float p[3], c[3];
        fallbacks += place_group(placement, pos, col, T, inc_start.data(), inc.data(), cell, Members{order.data() + begin}, (int64_t)(end - begin), p, c) ? 1 : 0;
        for (int a = 0; a < 3; a++) {
            uint32_t u;
            memcpy(&u, &p[a], 4); opos[3 * o + a] = u;
            memcpy(&u, &c[a], 4); ocol[3 * o + a] = u;
        }
    }
    // ---- k_ts_vertices, k_ts_triangles ----
    std::vector<int64_t> vmap(nv), vi, ti, tr;
    for (int64_t v = 0; v < nv; v++) {
        const int64_t r = rep[v];
        const bool kept = vnew[r + 1] != vnew[r];
        vmap[v] = wld::map_of(kept, (uint32_t)vnew[r]);
        if (r == v && kept) vi.push_back(v);
    }
    for (int64_t t = 0; t < nt; t++)
        if (tflag[t]) {
            ti.push_back(t);
            for (int k = 0; k < 3; k++) tr.push_back(vnew[rep[T[3 * t + k]]]);
        }
    const std::vector<int64_t> first = {0, kv, kt, nv - groups, degenerate, nt - degenerate - kt, groups - kv, passes + triangle_passes(groups, flags), fallbacks};
    put(out, first); put(out, vmap); put(out, vi); put(out, ti); put(out, tr); put(out, opos); put(out, ocol);
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
    if (mode == "simplify") {
        rc = simplify(in, out);
    } else if (mode == "args") {
        for (size_t i = 0; i + 11 < in.size(); i += 12) {
            float cell;
            int32_t pf[2];
            memcpy(&cell, in.data() + i, 4);
            memcpy(pf, in.data() + i + 4, 8);
            const int32_t o[4] = {cell_is_valid(cell), placement_is_valid(pf[0]), flags_are_known(pf[1]), flags_are_compatible(pf[1])};
            fwrite(o, 4, 4, out);
        }
    } else if (mode == "triple") {
        const uint32_t* p = (const uint32_t*)in.data();
        for (size_t i = 0; i + 3 < in.size() / 4; i += 4) {
            const Triple t = sorted_triple(p[i], p[i + 1], p[i + 2]);
            const uint64_t o[8] = {t.lo, t.mid, t.hi, has_vertex_set(t) ? 1u : 0u, triple_key_first(t), triple_key_second(t),
                                   triple_mask_first(p[i + 3]), triple_mask_second(p[i + 3])};
            fwrite(o, 8, 8, out);
        }
    } else if (mode == "run") {
        const int32_t* p = (const int32_t*)in.data();
        for (size_t i = 0; i + 3 < in.size() / 4; i += 4) {
            const int32_t o = keeps_in_run(p[i] != 0, p[i + 1] != 0, (uint32_t)p[i + 2], p[i + 3]) ? 1 : 0;
            fwrite(&o, 4, 1, out);
        }
    } else if (mode == "cell") {
        const double* p = (const double*)in.data();
        for (size_t i = 0; i + 2 < in.size() / 8; i += 3) {
            const int32_t o = in_cell(p[i], p[i + 1], (float)p[i + 2]) ? 1 : 0;
            fwrite(&o, 4, 1, out);
        }
    } else {
        rc = 1;
    }
    fclose(out);
    if (rc == 0) printf("mesh simplify ok\n");
    return rc;
}
