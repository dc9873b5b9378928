// mesh_winding_host.cpp -- runs sdfkit_amd/csrc/trimesh_winding.h (the lattice, the moments, the acceptance test, the stated atan2 and
// THE WALK the kernels of lib_trimesh_winding.hip run) on the host, over a hierarchy rebuilt as the library builds it (records sorted
// by (code, index), cells summed in sorted order, parents from their children in child order, radii as maxima), for
// tests/test_mesh_winding_host.py to compare with the numpy model.  The program also runs the header's own brute loop -- every triangle
// term in sorted order -- and counts the queries on which the walk with beta = +inf differs from it.
// usage: mesh_winding_host in out
//   in:  int64 nv, nt, n; f32 beta, 0; f32 V[3 nv]; int32 T[3 nt]; f32 Q[3 n]
//   out (int64): L, nodes with triangles, triangles in the fullest cell, cluster terms, triangle terms, queries where walk(+inf) != brute
//                loop, n, nodes in all; per query: the bits of w, inside, cluster terms, triangle terms; per node: count, start,
//                the bits of N[3], P[3], r2
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/trimesh_winding.h"

using namespace sdfk_trimesh_wn;

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

static int64_t bits(double x)
{
    int64_t u;
    memcpy(&u, &x, 8);
    return u;
}

struct HostTris {
    const float* V;
    const int32_t* T;
    void corners(uint32_t t, float a[3], float b[3], float c[3]) const
    {
        for (int k = 0; k < 3; k++) {
            a[k] = V[3 * (int64_t)T[3 * (int64_t)t] + k];
            b[k] = V[3 * (int64_t)T[3 * (int64_t)t + 1] + k];
            c[k] = V[3 * (int64_t)T[3 * (int64_t)t + 2] + k];
        }
    }
};

struct HostTree {
    int L = 0;
    std::vector<Node> nodes;
    std::vector<uint32_t> order;
    int64_t occupied = 0, max_leaf = 0;
};

static void build(HostTree& H, const HostTris& T, int64_t nt)
{
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t t = 0; t < nt; t++) {
        float p[3][3];
        T.corners((uint32_t)t, p[0], p[1], p[2]);
        for (int v = 0; v < 3; v++)
            for (int a = 0; a < 3; a++) {
                lo[a] = fminf(lo[a], p[v][a]);
                hi[a] = fmaxf(hi[a], p[v][a]);
            }
    }
    const Lattice A = lattice_for(lo, hi, nt);
    const int L = H.L = A.L;
    const uint32_t total = node_total(L), first = level_offset(L), cells = 1u << (3 * L);
    std::vector<uint32_t> code((size_t)nt);
    for (int64_t t = 0; t < nt; t++) {
        float a[3], b[3], c[3];
        double ctr[3];
        T.corners((uint32_t)t, a, b, c);
        tri_centroid(a, b, c, ctr);
        code[t] = leaf_code(A, ctr);
    }
    H.order.resize((size_t)nt);
    for (int64_t t = 0; t < nt; t++) H.order[t] = (uint32_t)t;
    std::stable_sort(H.order.begin(), H.order.end(), [&](uint32_t x, uint32_t y) { return code[x] < code[y]; });
    H.nodes.assign(total, Node{});
    std::vector<Sums> sums(total, no_sums());
    std::vector<uint32_t> starts(cells + 1, 0);
    for (int64_t t = 0; t < nt; t++) starts[code[t] + 1]++;
    for (uint32_t m = 0; m < cells; m++) starts[m + 1] += starts[m];
    for (uint32_t m = 0; m < cells; m++) {
        Sums S = no_sums();
        for (uint32_t j = starts[m]; j < starts[m + 1]; j++) {
            float a[3], b[3], c[3];
            T.corners(H.order[j], a, b, c);
            add_triangle(S, a, b, c);
        }
        sums[first + m] = S;
        H.nodes[first + m].start = starts[m];
        H.nodes[first + m].count = starts[m + 1] - starts[m];
    }
    for (int l = L - 1; l >= 0; l--)
        for (uint32_t i = 0; i < (1u << (3 * l)); i++) {
            const uint32_t node = level_offset(l) + i, child = 8 * node + 1;
            Sums S = no_sums();
            uint32_t count = 0;
            for (uint32_t c = 0; c < 8; c++) {
                add_sums(S, sums[child + c]);
                count += H.nodes[child + c].count;
            }
            sums[node] = S;
            H.nodes[node].start = H.nodes[child].start;
            H.nodes[node].count = count;
        }
    for (uint32_t node = 0; node < total; node++) {
        Node& nd = H.nodes[node];
        double N[3] = {0.0, 0.0, 0.0}, P[3] = {0.0, 0.0, 0.0};
        if (nd.count) {
            float a[3], b[3], c[3];
            double ctr[3];
            T.corners(H.order[nd.start], a, b, c);
            tri_centroid(a, b, c, ctr);
            node_moments(sums[node], ctr, N, P);
            H.occupied++;
            if (node >= first) H.max_leaf = std::max<int64_t>(H.max_leaf, nd.count);
        }
        for (int k = 0; k < 3; k++) { nd.N[k] = N[k]; nd.P[k] = P[k]; }
        nd.r2 = 0.0;
    }
    for (int l = 0; l <= L; l++)
        for (int64_t t = 0; t < nt; t++) {
            Node& nd = H.nodes[level_offset(l) + (code[t] >> (3 * (L - l)))];
            float v[3][3];
            T.corners((uint32_t)t, v[0], v[1], v[2]);
            for (int k = 0; k < 3; k++) nd.r2 = std::max(nd.r2, vertex_r2(v[k], nd.P));
        }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::vector<char> in = slurp(argv[1]);
    int64_t h[3];
    float r[2];
    if (in.size() < sizeof h + sizeof r) return 3;
    memcpy(h, in.data(), sizeof h);
    memcpy(r, in.data() + sizeof h, sizeof r);
    const int64_t nv = h[0], nt = h[1], n = h[2];
    if (nt < 1 || in.size() != sizeof h + sizeof r + 4 * (size_t)(3 * nv + 3 * nt + 3 * n)) return 3;
    const float* V = (const float*)(in.data() + sizeof h + sizeof r);
    const int32_t* Tr = (const int32_t*)(V + 3 * nv);
    const float* Q = (const float*)(Tr + 3 * nt);
    const HostTris T{V, Tr};
    HostTree H;
    build(H, T, nt);
    const double beta = (double)r[0], beta2 = beta * beta;
    std::vector<int64_t> out(8, 0);
    out[0] = H.L; out[1] = H.occupied; out[2] = H.max_leaf; out[6] = n; out[7] = (int64_t)H.nodes.size();
    for (int64_t i = 0; i < n; i++) {
        const float* qf = Q + 3 * i;
        Counts K{0, 0};
        const double w = winding(H.nodes.data(), H.order.data(), T, H.L, qf, beta2, K);
        out[3] += (int64_t)K.clusters;
        out[4] += (int64_t)K.triangles;
        // the same code's brute loop against the walk without approximation
        Counts Kinf{0, 0};
        const double winf = winding(H.nodes.data(), H.order.data(), T, H.L, qf, (double)INFINITY, Kinf);
        double wb = __builtin_nan("");
        if (finite32(qf[0]) && finite32(qf[1]) && finite32(qf[2])) {
            const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
            wb = 0.0;
            for (int64_t j = 0; j < nt; j++) {
                float a[3], b[3], c[3];
                T.corners(H.order[j], a, b, c);
                wb = wb + triangle_term(a, b, c, q);
            }
            if (bits(wb) != bits(winf) || Kinf.clusters != 0 || (int64_t)Kinf.triangles != nt) out[5]++;
        } else if (winf == winf)
            out[5]++;
        out.insert(out.end(), {w != w ? bits(__builtin_nan("")) : bits(w), (int64_t)inside_of(w), (int64_t)K.clusters, (int64_t)K.triangles});
    }
    for (const Node& nd : H.nodes)
        out.insert(out.end(), {(int64_t)nd.count, (int64_t)nd.start, bits(nd.N[0]), bits(nd.N[1]), bits(nd.N[2]), bits(nd.P[0]), bits(nd.P[1]),
                               bits(nd.P[2]), bits(nd.r2)});
    FILE* f = fopen(argv[2], "wb");
    if (!f) return 4;
    fwrite(out.data(), sizeof(int64_t), out.size(), f);
    fclose(f);
    printf("mesh winding ok\n");
    return 0;
}
