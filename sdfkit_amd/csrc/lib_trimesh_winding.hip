// lib_trimesh_winding.hip -- the generalized winding number of triangle meshes: sdfk_trimesh_winding (w and "inside" of arbitrary
// points) and sdfk_trimesh_to_volume_signed (sdfk_trimesh_to_volume with the sign taken from w).  Contract: include/sdfkit_hip.h,
// "Triangle meshes: generalized winding number".  Arithmetic, the hierarchy and the walk: trimesh_winding.h (shared with a host test,
// which runs the same code).
//
// Build (the first call that needs it; kept on the handle): one record (cell code, index) per triangle, sorted by device_sort.h --
// stable, so equal codes stay in index order -- while integer atomics count the triangles of every cell; a scan of the counts gives
// the cells' runs.  One lane per cell of level L adds its run's moments in sorted order; one lane per node of each level above adds
// its eight children's; one lane per node makes N and P; one lane per (sorted triangle, level) raises its ancestor's r2 with an
// integer atomicMax on the bits of the non-negative binary64 value (a maximum: order-free).  The dense levels make a node's children,
// parent and successor arithmetic on its number, so the walk needs no stack.
// Query: one lane per query, 256-lane blocks; the lane adds its terms in the walk's order, so nothing depends on other lanes.
// Volume: a sign pass with lanes along z, as k_tm_volume runs (a wave's queries are neighbours and open the same nodes), writes one
// byte per voxel; trimesh_to_volume (lib_trimesh.hip) then runs its one volume pass reading that byte in place of the crossings.
// A sign pass, not a template parameter of k_tm_volume: the walk and the closest-triangle search are both long binary64 loops
// with their own live state, and one kernel holding both would carry the registers of both for the whole of its run.
#include "lib_internal.h"
#include "device_sort.h"
#include "device_wave.h"
#include "trimesh_handle.h"
#include "trimesh_sdf.h"
#include "trimesh_winding.h"

namespace {

using namespace sdfk_trimesh_wn;
using sdfk_trimesh_sdf::col_coord;

constexpr int kBlock = 256;

// ---- build ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_wn_keys(const TriPack* __restrict__ tri, int64_t nt, Lattice A, Rec* __restrict__ rec,
                                                    uint32_t* __restrict__ cnt)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    float a[3], b[3], c[3];
    double ctr[3];
    PackTris{tri}.corners((uint32_t)t, a, b, c);
    tri_centroid(a, b, c, ctr);
    const uint32_t m = leaf_code(A, ctr);
    rec[t] = Rec{m, (uint32_t)t, 0u};
    atomicAdd(&cnt[m], 1u);
}

__global__ __launch_bounds__(kBlock) void k_wn_order(const Rec* __restrict__ sorted, int64_t nt, uint32_t* __restrict__ order)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < nt) order[j] = sorted[j].index;
}

// the cells of level L: their runs and the sums over them, in sorted order
__global__ __launch_bounds__(kBlock) void k_wn_cells(const TriPack* __restrict__ tri, const uint32_t* __restrict__ order,
                                                     const uint32_t* __restrict__ starts, uint32_t cells, uint32_t first, Node* __restrict__ nodes,
                                                     Sums* __restrict__ sums)
{
    const uint32_t m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= cells) return;
    const uint32_t j0 = starts[m], j1 = starts[m + 1];
    Sums S = no_sums();
    const PackTris T{tri};
    for (uint32_t j = j0; j < j1; j++) {
        float a[3], b[3], c[3];
        T.corners(order[j], a, b, c);
        add_triangle(S, a, b, c);
    }
    sums[first + m] = S;
    nodes[first + m].start = j0;
    nodes[first + m].count = j1 - j0;
}

// the nodes [first, first + n) of one level above the cells, from their children
__global__ __launch_bounds__(kBlock) void k_wn_up(uint32_t first, uint32_t n, Node* __restrict__ nodes, Sums* __restrict__ sums)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t node = first + i, child = 8 * node + 1;
    Sums S = no_sums();
    uint32_t count = 0;
    for (uint32_t c = 0; c < 8; c++) {
        add_sums(S, sums[child + c]);
        count += nodes[child + c].count;
    }
    sums[node] = S;
    nodes[node].start = nodes[child].start;
    nodes[node].count = count;
}

__global__ __launch_bounds__(kBlock) void k_wn_moments(const TriPack* __restrict__ tri, const uint32_t* __restrict__ order, uint32_t total,
                                                       uint32_t first_cell, Node* __restrict__ nodes, const Sums* __restrict__ sums,
                                                       unsigned long long* __restrict__ census)
{
    const uint32_t node = blockIdx.x * kBlock + threadIdx.x;
    if (node >= total) return;
    Node& nd = nodes[node];
    double N[3] = {0.0, 0.0, 0.0}, P[3] = {0.0, 0.0, 0.0};
    if (nd.count) {
        float a[3], b[3], c[3];
        double ctr[3];
        PackTris{tri}.corners(order[nd.start], a, b, c);
        tri_centroid(a, b, c, ctr);
        node_moments(sums[node], ctr, N, P);
        atomicAdd(&census[0], 1ull);
        if (node >= first_cell) atomicMax(&census[1], (unsigned long long)nd.count);
    }
    for (int k = 0; k < 3; k++) { nd.N[k] = N[k]; nd.P[k] = P[k]; }
    nd.r2 = 0.0;
}

// one lane per (sorted position, level): the three vertices against the ancestor's P
__global__ __launch_bounds__(kBlock) void k_wn_radius(const TriPack* __restrict__ tri, const Rec* __restrict__ sorted, int64_t nt, int L,
                                                      Node* __restrict__ nodes)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nt * (L + 1)) return;
    const int l = (int)(i / nt);
    const Rec r = sorted[i - (int64_t)l * nt];
    Node& nd = nodes[level_offset(l) + (uint32_t)(r.key >> (3 * (L - l)))];
    float v[3][3];
    PackTris{tri}.corners(r.index, v[0], v[1], v[2]);
    const double P[3] = {nd.P[0], nd.P[1], nd.P[2]};
    double m = vertex_r2(v[0], P);
    m = fmax(m, vertex_r2(v[1], P));
    m = fmax(m, vertex_r2(v[2], P));
    atomicMax((unsigned long long*)&nd.r2, (unsigned long long)__double_as_longlong(m));   // (m >= 0: its bits order as it does)
}

// ---- queries ----------------------------------------------------------------------------------------------------------------
struct Tree {
    const Node* nodes;
    const uint32_t* order;
    const TriPack* tri;
    int L;
    double beta2;
};

// (terms: the two words of a profiled call, or null)
__device__ __forceinline__ void count_terms(unsigned long long* terms, const Counts& K)
{
    if (!terms) return;
    wave_add(&terms[0], K.clusters);
    wave_add(&terms[1], K.triangles);
}

__global__ __launch_bounds__(kBlock) void k_wn_query(Tree S, const float* __restrict__ queries, int64_t n, float* __restrict__ winding,
                                                     uint8_t* __restrict__ inside, unsigned long long* __restrict__ terms)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool active = i < n;
    float q[3] = {NAN, NAN, NAN};   // (an idle lane walks nothing)
    if (active)
        for (int a = 0; a < 3; a++) q[a] = queries[3 * i + a];
    Counts K{0, 0};
    const double w = sdfk_trimesh_wn::winding(S.nodes, S.order, PackTris{S.tri}, S.L, q, S.beta2, K);
    count_terms(terms, K);
    if (!active) return;
    if (winding) winding[i] = winding_f32(w);
    if (inside) inside[i] = inside_of(w) ? 1 : 0;
}

struct SignArgs {
    int nx, ny, nz, z0;
    float mx, my, mz, dx, dy, dz;
};

// the sign bytes of a volume, in k_tm_volume's order (z fastest, unpadded) at k_tm_volume's cell centres
__global__ __launch_bounds__(kBlock) void k_wn_volume_sign(Tree S, SignArgs A, uint8_t* __restrict__ sign, unsigned long long* __restrict__ terms)
{
    const int64_t n = (int64_t)A.nx * A.ny * A.nz;
    const int64_t g0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool active = g0 < n;
    float q[3] = {NAN, NAN, NAN};
    if (active) {
        const int k = (int)(g0 % A.nz);
        const int64_t row = g0 / A.nz;   // = i * ny + j
        const int j = (int)(row % A.ny), i = (int)(row / A.ny);
        q[0] = col_coord(A.mx, i, A.dx);
        q[1] = col_coord(A.my, j, A.dy);
        q[2] = col_coord(A.mz, A.z0 + k, A.dz);
    }
    Counts K{0, 0};
    const double w = sdfk_trimesh_wn::winding(S.nodes, S.order, PackTris{S.tri}, S.L, q, S.beta2, K);
    count_terms(terms, K);
    if (active) sign[g0] = inside_of(w) ? 1 : 0;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
int winding_build(sdfk_trimesh* t, const char* who)
{
    if (t->wn_nodes) return SDFK_OK;
    const int64_t nt = t->nt;
    const Lattice A = lattice_for(t->G.lo, t->G.hi, nt);
    const int L = A.L;
    const uint32_t total = node_total(L), first_cell = level_offset(L), cells = 1u << (3 * L);
    const unsigned mask = (1u << ((3 * L + 7) / 8)) - 1u;   // the radix passes that the 3 L bits of a code need
    Staged st;
    Node* nodes = st.kept<Node>(total);
    uint32_t* order = st.kept<uint32_t>((size_t)nt);
    Sums* sums = st.scratch<Sums>(total);
    uint32_t* cnt = st.scratch<uint32_t>((size_t)cells + 1);
    Rec* ra = st.scratch<Rec>((size_t)nt);
    Rec* rb = st.scratch<Rec>((size_t)nt);
    unsigned long long* census = st.scratch<unsigned long long>(2);
    Rec* sorted = nullptr;
    unsigned long long host[2] = {0, 0};
    st.run([&] { return hipMemsetAsync(cnt, 0, ((size_t)cells + 1) * sizeof(uint32_t), g.stream); });
    st.run([&] { return hipMemsetAsync(census, 0, 2 * sizeof(unsigned long long), g.stream); });
    st.run([&] {
        ProfScope ps("k_wn_keys");
        hipLaunchKernelGGL(k_wn_keys, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->tri, nt, A, ra, cnt);
    });
    st.run([&] { return radix_sort(ra, rb, nt, mask, &sorted, who); });
    st.run([&] { return sdfk_scan::scan(cnt, (int64_t)cells, who); });
    st.run([&] {
        ProfScope ps("k_wn_build");
        hipLaunchKernelGGL(k_wn_order, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, sorted, nt, order);
        hipLaunchKernelGGL(k_wn_cells, dim3(grid1(cells)), dim3(kBlock), 0, g.stream, t->tri, order, cnt, cells, first_cell, nodes, sums);
        for (int l = L - 1; l >= 0; l--) {
            const uint32_t n = 1u << (3 * l);
            hipLaunchKernelGGL(k_wn_up, dim3(grid1(n)), dim3(kBlock), 0, g.stream, level_offset(l), n, nodes, sums);
        }
        hipLaunchKernelGGL(k_wn_moments, dim3(grid1(total)), dim3(kBlock), 0, g.stream, t->tri, order, total, first_cell, nodes, sums, census);
        hipLaunchKernelGGL(k_wn_radius, dim3(grid1(nt * (L + 1))), dim3(kBlock), 0, g.stream, t->tri, sorted, nt, L, nodes);
    });
    st.read(host, census, sizeof host);   // (synchronises: the build is done when the first query is queued)
    if (int r = st.finish(who, false)) return r;
    t->wn_nodes = nodes;
    t->wn_order = order;
    t->wn_levels = L;
    t->wn_occupied = (int64_t)host[0];
    t->wn_max_leaf = (int64_t)host[1];
    t->wn_builds++;
    return SDFK_OK;
}

Tree tree_of(const sdfk_trimesh* t, float beta) { return Tree{(const Node*)t->wn_nodes, t->wn_order, t->tri, t->wn_levels, (double)beta * (double)beta}; }

// the two term counts of a profiled call, onto the handle
void keep_terms(Staged& st, ProfCount<2>& pc, sdfk_trimesh* t, int64_t queries)
{
    unsigned long long c[2];
    if (!pc.end(st, c)) return;
    t->last_wn_clusters = (int64_t)c[0];
    t->last_wn_triangles = (int64_t)c[1];
    t->last_wn_queries = queries;
}

int winding_check(const sdfk_trimesh* t, const void* queries, int64_t n, float beta, const char* who)
{
    if (int r = trimesh_check(t, who, 1)) return r;
    if (n < 0) return fail(SDFK_ERR_INVALID, "%s: n must be >= 0", who);
    if (n >= (int64_t(1) << 32)) return fail(SDFK_ERR_INVALID, "%s: 2^32 queries or more", who);
    if (!(beta >= 0.0f)) return fail(SDFK_ERR_INVALID, "%s: beta must be >= 0 (+inf: no approximation)", who);
    if (n > 0 && !queries) return fail(SDFK_ERR_INVALID, "%s: null queries", who);
    return SDFK_OK;
}

int winding_launch(sdfk_trimesh* t, const float* q, int64_t n, float beta, float* winding, uint8_t* inside, const char* who)
{
    Staged st;
    ProfCount<2> pc;
    pc.begin(st);
    st.run([&] {
        ProfScope ps("k_wn_query");
        hipLaunchKernelGGL(k_wn_query, dim3(grid1(n)), dim3(kBlock), 0, g.stream, tree_of(t, beta), q, n, winding, inside, pc.dev);
    });
    keep_terms(st, pc, t, n);
    return st.finish(who, false);
}

int volume_winding(sdfk_trimesh* t, sdfk_volume* v, float band, float beta, const char* who)
{
    if (v->elided || !v->values) return fail(SDFK_ERR_INVALID, "%s: the volume has no storage", who);
    if (int r = winding_build(t, who)) return r;
    float d[3], m[3], outside;
    grid_constants(v, d, m, &outside);
    const int64_t n = (int64_t)v->nx * v->ny * v->nz;
    Staged st;
    uint8_t* sign = st.scratch<uint8_t>((size_t)n);
    ProfCount<2> pc;
    pc.begin(st);
    st.run([&] {
        const SignArgs A{v->nx, v->ny, v->nz, v->z0, m[0], m[1], m[2], d[0], d[1], d[2]};
        ProfScope ps("k_wn_volume_sign");
        hipLaunchKernelGGL(k_wn_volume_sign, dim3(grid1(n)), dim3(kBlock), 0, g.stream, tree_of(t, beta), A, sign, pc.dev);
    });
    keep_terms(st, pc, t, n);
    st.run([&] { return trimesh_to_volume(t, v, band, sign); });
    return st.finish(who, false);   // (the bytes go back to the stream-ordered pool under the queued volume pass)
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_trimesh_winding_device(sdfk_trimesh* t, const void* queries3_dev, int64_t n, float beta, void* winding_dev, void* inside_dev)
{
    static const char* who = "sdfk_trimesh_winding";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = winding_check(t, queries3_dev, n, beta, who)) return r;
    if (n == 0) return SDFK_OK;
    if (int r = winding_build(t, who)) return r;
    return winding_launch(t, (const float*)queries3_dev, n, beta, (float*)winding_dev, (uint8_t*)inside_dev, who);
}

extern "C" int sdfk_trimesh_winding(sdfk_trimesh* t, const float* queries3, int64_t n, float beta, float* winding, uint8_t* inside)
{
    static const char* who = "sdfk_trimesh_winding";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = winding_check(t, queries3, n, beta, who)) return r;
    if (n == 0) return SDFK_OK;
    if (int r = winding_build(t, who)) return r;
    Staged st;
    const float* qd = st.in(queries3, (size_t)n * 3);
    float* wd = st.out(winding, (size_t)n);
    uint8_t* id = st.out(inside, (size_t)n);
    st.run([&] { return winding_launch(t, qd, n, beta, wd, id, who); });
    return st.finish(who);
}

extern "C" int sdfk_trimesh_to_volume_signed(sdfk_trimesh* t, sdfk_volume* v, float max_distance, int32_t sign_mode, float beta)
{
    static const char* who = "sdfk_trimesh_to_volume_signed";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = trimesh_check(t, who, 1)) return r;
    if (!v) return fail(SDFK_ERR_INVALID, "%s: null argument", who);
    if (!(max_distance >= 0.0f)) return fail(SDFK_ERR_INVALID, "%s: max_distance must be >= 0 (+inf: exact everywhere)", who);
    if (sign_mode == SDFK_TRIMESH_SIGN_PARITY) return trimesh_to_volume(t, v, max_distance, nullptr);
    if (sign_mode != SDFK_TRIMESH_SIGN_WINDING) return fail(SDFK_ERR_INVALID, "%s: unknown sign_mode %d", who, (int)sign_mode);
    if (!(beta >= 0.0f)) return fail(SDFK_ERR_INVALID, "%s: beta must be >= 0 (+inf: no approximation)", who);
    return volume_winding(t, v, max_distance, beta, who);
}

extern "C" int sdfk_trimesh_winding_stats(const sdfk_trimesh* t, int64_t stats[8])
{
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!t || !stats) return fail(SDFK_ERR_INVALID, "sdfk_trimesh_winding_stats: null argument");
    stats[0] = t->wn_levels;
    stats[1] = t->wn_occupied;
    stats[2] = t->wn_max_leaf;
    stats[3] = t->wn_builds;
    stats[4] = t->last_wn_clusters;
    stats[5] = t->last_wn_triangles;
    stats[6] = t->last_wn_queries;
    stats[7] = t->wn_levels >= 0 ? (int64_t)node_total(t->wn_levels) : 0;
    return SDFK_OK;
}
