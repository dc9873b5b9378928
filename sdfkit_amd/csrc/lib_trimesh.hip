// lib_trimesh.hip -- signed distance volumes from triangle meshes (Mesh -> Voxels): exact closest-triangle search and crossing
// parity along z.  Contract: include/sdfkit_hip.h, "Triangle-mesh distance".  Arithmetic: trimesh_sdf.h (shared with a host test).
//
// Build (create): the triangles are validated and packed on the device (vertices + f32 AABB, 64 bytes each), then binned into
// every cell of a uniform grid (points_grid.h, sized from the triangle count) that their AABB overlaps, by count, scan
// (device_scan.h) and scatter.  Two prefix arrays describe the cells: `starts` in x-fastest order (a run of x cells is one contiguous range of the
// sorted list) and `ystarts` in y-fastest order (a run of y cells can be tested for emptiness with two loads).
// Search: one lane per query, cells in growing Chebyshev shells, each shell as its six faces: z and y faces as x runs, x faces as
// y runs skipped when empty.  It stops when a conservative f32 lower bound on every unvisited cell exceeds the best d2 (or the
// band).  An f32 AABB bound rejects candidates before the binary64 closest-point routine.
// Sign: every triangle with a nonzero exact projected area is tested against the columns of its xy box -- one lane per
// (triangle, column) item, the items of all triangles flattened by a scan, so a triangle over 10^5 columns is spread over 10^5
// lanes -- count, scan, write: crossing records grouped by column.  The volume pass runs one lane per voxel (z fastest) and
// counts the crossings of its column below it.
// Sample (sdfk_trimesh_sample; arithmetic: trimesh_sample.h): the first call makes the integer weights of the triangles (area over
// the largest area, in units of 2^-32) and their exclusive 64-bit scan W, kept on the handle; every call runs one lane per sample:
// three stateless draws, a binary search over W, one TriPack gather, the stores.
// The handle (struct sdfk_trimesh, TriPack) is in trimesh_handle.h, shared with lib_trimesh_topology.hip, which reads W as well, with
// lib_trimesh_smooth.hip, lib_trimesh_weld.hip, lib_trimesh_simplify.hip and lib_trimesh_ray.hip (which walks the grid along
// rays); trimesh_check, the check of a handle that all of them begin with, is defined here.
// Host side: every work function holds its scratch, and every host form its device copies, in a Staged (device_stage.h).
#include "lib_internal.h"
#include "device_scan.h"
#include "device_wave.h"
#include "points_grid.h"
#include "trimesh_handle.h"
#include "trimesh_sdf.h"
#include "trimesh_sample.h"

#include <cfloat>

namespace {

using namespace sdfk_points_grid;   // Grid, cell_of, grid_for_box
using namespace sdfk_trimesh_sdf;
namespace smp = sdfk_trimesh_smp;

constexpr int kBlock = 256;

// ---- build ------------------------------------------------------------------------------------------------------------------
// flags[0]: indices out of range, flags[1]: non-finite vertex coordinates
__global__ __launch_bounds__(kBlock) void k_tm_vcheck(const float* __restrict__ v, int64_t nv, unsigned* __restrict__ flags)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < 3 * nv; i += (int64_t)gridDim.x * kBlock)
        if (!isfinite(v[i])) atomicOr(&flags[1], 1u);
}

__global__ __launch_bounds__(kBlock) void k_tm_pack(const float* __restrict__ v, int64_t nv, const int32_t* __restrict__ idx, int64_t nt,
                                                    TriPack* __restrict__ tri, unsigned* __restrict__ flags)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    float p[3][3];
    bool ok = true;
    for (int k = 0; k < 3; k++) {
        const int32_t i = idx[3 * t + k];
        if (i < 0 || (int64_t)i >= nv) { ok = false; p[k][0] = p[k][1] = p[k][2] = 0.0f; continue; }
        p[k][0] = v[3 * (int64_t)i]; p[k][1] = v[3 * (int64_t)i + 1]; p[k][2] = v[3 * (int64_t)i + 2];
    }
    if (!ok) atomicOr(&flags[0], 1u);
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = fminf(fminf(p[0][a], p[1][a]), p[2][a]);
        hi[a] = fmaxf(fmaxf(p[0][a], p[1][a]), p[2][a]);
    }
    TriPack P;
    P.p0 = make_float4(p[0][0], p[0][1], p[0][2], p[1][0]);
    P.p1 = make_float4(p[1][1], p[1][2], p[2][0], p[2][1]);
    P.p2 = make_float4(p[2][2], lo[0], lo[1], lo[2]);
    P.p3 = make_float4(hi[0], hi[1], hi[2], 0.0f);
    tri[t] = P;
}

// per-block min / max of the triangle AABBs -> part[block][6]; then one block -> out[6]
__global__ __launch_bounds__(kBlock) void k_tm_bounds(const TriPack* __restrict__ tri, int64_t nt, float* __restrict__ part, int final_pass)
{
    __shared__ float s[6][kBlock];
    float r[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (!final_pass) {
        for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < nt; t += (int64_t)gridDim.x * kBlock) {
            const float4 a = tri[t].p2, b = tri[t].p3;
            r[0] = fminf(r[0], a.y); r[1] = fminf(r[1], a.z); r[2] = fminf(r[2], a.w);
            r[3] = fmaxf(r[3], b.x); r[4] = fmaxf(r[4], b.y); r[5] = fmaxf(r[5], b.z);
        }
    } else {
        for (int64_t b = threadIdx.x; b < nt; b += kBlock)   // (nt = the number of partials here)
            for (int j = 0; j < 6; j++) r[j] = j < 3 ? fminf(r[j], part[8 * b + j]) : fmaxf(r[j], part[8 * b + j]);
    }
    for (int j = 0; j < 6; j++) s[j][threadIdx.x] = r[j];
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            for (int j = 0; j < 3; j++) s[j][threadIdx.x] = fminf(s[j][threadIdx.x], s[j][threadIdx.x + o]);
            for (int j = 3; j < 6; j++) s[j][threadIdx.x] = fmaxf(s[j][threadIdx.x], s[j][threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) part[(final_pass ? 8 * 1024 : 8 * (int64_t)blockIdx.x) + threadIdx.x] = s[threadIdx.x][0];
}

__device__ __forceinline__ void tri_cells(const TriPack& P, const Grid& G, int c0[3], int c1[3])
{
    const float lo[3] = {P.p2.y, P.p2.z, P.p2.w}, hi[3] = {P.p3.x, P.p3.y, P.p3.z};
    for (int a = 0; a < 3; a++) {
        c0[a] = cell_of(lo[a], G.lo[a], G.inv_h, G.dim[a]);
        c1[a] = cell_of(hi[a], G.lo[a], G.inv_h, G.dim[a]);
    }
}

// per-cell counts of the binned triangles, and their total (u64)
__global__ __launch_bounds__(kBlock) void k_tm_bin_count(const TriPack* __restrict__ tri, int64_t nt, Grid G, uint32_t* __restrict__ counts,
                                                         unsigned long long* __restrict__ total)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long n = 0;
    if (t < nt) {
        int c0[3], c1[3];
        tri_cells(tri[t], G, c0, c1);
        for (int z = c0[2]; z <= c1[2]; z++)
            for (int y = c0[1]; y <= c1[1]; y++)
                for (int x = c0[0]; x <= c1[0]; x++) atomicAdd(&counts[((uint32_t)z * (uint32_t)G.dim[1] + (uint32_t)y) * (uint32_t)G.dim[0] + (uint32_t)x], 1u);
        n = (unsigned long long)(c1[0] - c0[0] + 1) * (unsigned long long)(c1[1] - c0[1] + 1) * (unsigned long long)(c1[2] - c0[2] + 1);
    }
    n = wave_sum(n);   // (total is never null: no test of it, unlike wave_add)
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(total, n);
}

__global__ __launch_bounds__(kBlock) void k_tm_bin_scatter(const TriPack* __restrict__ tri, int64_t nt, Grid G, uint32_t* __restrict__ cursor,
                                                           uint32_t* __restrict__ list)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    int c0[3], c1[3];
    tri_cells(tri[t], G, c0, c1);
    for (int z = c0[2]; z <= c1[2]; z++)
        for (int y = c0[1]; y <= c1[1]; y++)
            for (int x = c0[0]; x <= c1[0]; x++) {
                const uint32_t slot = atomicAdd(&cursor[((uint32_t)z * (uint32_t)G.dim[1] + (uint32_t)y) * (uint32_t)G.dim[0] + (uint32_t)x], 1u);
                list[slot] = (uint32_t)t;
            }
}

// cell counts in y-fastest order ((x * dimz + z) * dimy + y), from the x-fastest starts
__global__ __launch_bounds__(kBlock) void k_tm_ycounts(const uint32_t* __restrict__ starts, Grid G, int64_t cells, uint32_t* __restrict__ yc)
{
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= cells) return;
    const int64_t x = c % G.dim[0], y = (c / G.dim[0]) % G.dim[1], z = c / ((int64_t)G.dim[0] * G.dim[1]);
    yc[(x * G.dim[2] + z) * G.dim[1] + y] = starts[c + 1] - starts[c];
}

// ---- search -----------------------------------------------------------------------------------------------------------------
struct Best {
    double d2;
    int bi;
    Closest cl;
    unsigned long long ncand;
};

// (the corners of a TriPack the lane holds; by index from the array: PackTris, trimesh_handle.h)
__device__ __forceinline__ void load_tri(const TriPack& P, float a[3], float b[3], float c[3])
{
    a[0] = P.p0.x; a[1] = P.p0.y; a[2] = P.p0.z;
    b[0] = P.p0.w; b[1] = P.p1.x; b[2] = P.p1.y;
    c[0] = P.p1.z; c[1] = P.p1.w; c[2] = P.p2.x;
}

__device__ __forceinline__ void visit_range(const TriPack* __restrict__ tri, const uint32_t* __restrict__ list, uint32_t j0, uint32_t j1,
                                            const float q[3], const double qd[3], float slack, Best& B)
{
    for (uint32_t j = j0; j < j1; j++) {
        const uint32_t t = list[j];
        const TriPack P = tri[t];
        // f32 distance to the AABB, made conservative: each gap less the grid's absolute slack (which covers the binary64
        // closest point's absolute error, about |coordinates| 2^-52), the sum scaled by 1 - 2^-18 (a few relative roundings)
        const float gx = fmaxf(fmaxf(P.p2.y - q[0], q[0] - P.p3.x) - slack, 0.0f);
        const float gy = fmaxf(fmaxf(P.p2.z - q[1], q[1] - P.p3.y) - slack, 0.0f);
        const float gz = fmaxf(fmaxf(P.p2.w - q[2], q[2] - P.p3.z) - slack, 0.0f);
        const float lb = __fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)), __fmul_rn(gz, gz));
        if ((double)lb * (1.0 - 0x1p-18) > B.d2) continue;
        float a[3], b[3], c[3];
        load_tri(P, a, b, c);
        const double ad[3] = {a[0], a[1], a[2]}, bd[3] = {b[0], b[1], b[2]}, cd[3] = {c[0], c[1], c[2]};
        const Closest C = closest_on_triangle(qd, ad, bd, cd);
        B.ncand++;
        if (C.d2 < B.d2 || (C.d2 == B.d2 && (int)t < B.bi)) { B.d2 = C.d2; B.bi = (int)t; B.cl = C; }
    }
}

struct SearchGrid {
    const TriPack* tri;
    const uint32_t* list;
    const uint32_t* starts;
    const uint32_t* ystarts;
    Grid G;
};

__device__ __forceinline__ float lb_sq(const float gap[3][2], const float base2[3])
{
    float best = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float rest = base2[(a + 1) % 3] + base2[(a + 2) % 3];
        const float gm = fminf(gap[a][0], gap[a][1]);
        best = fminf(best, gm * gm + rest);
    }
    return best;
}

// The triangle of least (d2, index) for the finite query q.  The search may stop once every unvisited triangle is farther than
// stop2: the result is then exact whenever the least d2 is <= stop2, and otherwise some triangle with d2 > stop2 (or none).
__device__ void tm_search(const SearchGrid& S, const float q[3], double stop2, Best& B)
{
    const Grid& G = S.G;
    B.d2 = INFINITY;
    B.bi = -1;
    const double qd[3] = {q[0], q[1], q[2]};
    int c[3];
    for (int a = 0; a < 3; a++) c[a] = cell_of(q[a], G.lo[a], G.inv_h, G.dim[a]);
    const float slack = G.slack + fmaxf(fabsf(q[0]), fmaxf(fabsf(q[1]), fabsf(q[2]))) * 0x1p-20f;
    float base2[3];
    int rmax = 0;
    for (int a = 0; a < 3; a++) {
        const float out = fmaxf(fmaxf(G.lo[a] - q[a], q[a] - G.hi[a]) - slack, 0.0f);
        base2[a] = out * out;
        rmax = max(rmax, max(c[a], G.dim[a] - 1 - c[a]));
    }
    const int gx = G.dim[0], gy = G.dim[1], gz = G.dim[2];
    for (int r = 0; r <= rmax; r++) {
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, gx - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, gy - 1);
        const int zi0 = max(c[2] - r + 1, 0), zi1 = min(c[2] + r - 1, gz - 1);
        const int yi0 = max(c[1] - r + 1, 0), yi1 = min(c[1] + r - 1, gy - 1);
        // z faces: full x runs over y in [y0, y1]
        for (int side = 0; side < (r ? 2 : 1); side++) {
            const int z = side ? c[2] + r : c[2] - r;
            if (z < 0 || z >= gz) continue;
            for (int y = y0; y <= y1; y++) {
                const uint32_t row = ((uint32_t)z * (uint32_t)gy + (uint32_t)y) * (uint32_t)gx;
                visit_range(S.tri, S.list, S.starts[row + x0], S.starts[row + x1 + 1], q, qd, slack, B);
            }
        }
        if (r) {
            // y faces: full x runs over the inner z
            for (int side = 0; side < 2; side++) {
                const int y = side ? c[1] + r : c[1] - r;
                if (y < 0 || y >= gy) continue;
                for (int z = zi0; z <= zi1; z++) {
                    const uint32_t row = ((uint32_t)z * (uint32_t)gy + (uint32_t)y) * (uint32_t)gx;
                    visit_range(S.tri, S.list, S.starts[row + x0], S.starts[row + x1 + 1], q, qd, slack, B);
                }
            }
            // x faces: y runs over the inner z, skipped when empty
            if (yi0 <= yi1)
                for (int side = 0; side < 2; side++) {
                    const int x = side ? c[0] + r : c[0] - r;
                    if (x < 0 || x >= gx) continue;
                    for (int z = zi0; z <= zi1; z++) {
                        const uint32_t yrow = ((uint32_t)x * (uint32_t)gz + (uint32_t)z) * (uint32_t)gy;
                        if (S.ystarts[yrow + yi1 + 1] == S.ystarts[yrow + yi0]) continue;
                        for (int y = yi0; y <= yi1; y++) {
                            const uint32_t cell = ((uint32_t)z * (uint32_t)gy + (uint32_t)y) * (uint32_t)gx + (uint32_t)x;
                            visit_range(S.tri, S.list, S.starts[cell], S.starts[cell + 1], q, qd, slack, B);
                        }
                    }
                }
        }
        // every unvisited cell lies beyond shell r along some axis: the least distance it can have, made conservative
        float gap[3][2];
        for (int a = 0; a < 3; a++) {
            gap[a][0] = c[a] - r - 1 >= 0 ? fmaxf(q[a] - (G.lo[a] + (float)(c[a] - r) * G.h) - slack, 0.0f) : INFINITY;
            gap[a][1] = c[a] + r + 1 < G.dim[a] ? fmaxf((G.lo[a] + (float)(c[a] + r + 1) * G.h) - q[a] - slack, 0.0f) : INFINITY;
        }
        const double lb = (double)lb_sq(gap, base2) * (1.0 - 0x1p-18);
        if (lb > B.d2 || lb > stop2) break;
    }
}

// closest-triangle queries, caller order
struct QueryOut {
    int32_t* triangle;
    float* distance;
    float* closest3;
    unsigned long long* candidates;
};

__global__ __launch_bounds__(kBlock) void k_tm_closest(SearchGrid S, const float* __restrict__ queries, int64_t nq, QueryOut O)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool active = t < nq;
    Best B;
    B.bi = -1;
    B.ncand = 0;
    float q[3] = {NAN, NAN, NAN};
    if (active)
        for (int a = 0; a < 3; a++) q[a] = queries[3 * t + a];
    if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) tm_search(S, q, INFINITY, B);
    wave_add(O.candidates, B.ncand);
    if (!active) return;
    const bool found = B.bi >= 0;
    if (O.triangle) O.triangle[t] = B.bi;
    if (O.distance) O.distance[t] = found ? (float)__builtin_sqrt(B.d2) : INFINITY;
    if (O.closest3)
        for (int a = 0; a < 3; a++) O.closest3[3 * t + a] = found ? (float)B.cl.cp[a] : NAN;
}

// ---- crossings --------------------------------------------------------------------------------------------------------------
struct Columns {
    int nx, ny;
    float mx, my, dx, dy;   // column (i, j) is at (mx + i dx, my + j dy)
};

// per triangle: its column box and item count (0 for a zero projected area)
__global__ __launch_bounds__(kBlock) void k_tm_items(const TriPack* __restrict__ tri, int64_t nt, Columns Q, int4* __restrict__ box,
                                                     unsigned long long* __restrict__ items)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const TriPack P = tri[t];
    float a[3], b[3], c[3];
    load_tri(P, a, b, c);
    int i0 = 0, i1 = -1, j0 = 0, j1 = -1;
    if (projected_area_sign(a, b, c) != 0) {
        col_range(P.p2.y, P.p3.x, Q.mx, Q.dx, Q.nx, &i0, &i1);
        col_range(P.p2.z, P.p3.y, Q.my, Q.dy, Q.ny, &j0, &j1);
    }
    box[t] = make_int4(i0, i1, j0, j1);
    items[t] = (i1 >= i0 && j1 >= j0) ? (unsigned long long)(i1 - i0 + 1) * (unsigned long long)(j1 - j0 + 1) : 0ull;
}

// one lane per (triangle, column) item: pass 0 counts crossings per column, pass 1 writes their z
template <int PASS>
__global__ __launch_bounds__(kBlock) void k_tm_cross(const TriPack* __restrict__ tri, int64_t nt, Columns Q, const int4* __restrict__ box,
                                                     const unsigned long long* __restrict__ item_start, unsigned long long n_items,
                                                     uint32_t* __restrict__ col, double* __restrict__ zrec)
{
    for (unsigned long long it = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; it < n_items; it += (unsigned long long)gridDim.x * kBlock) {
        // the triangle: the last t with item_start[t] <= it
        int64_t lo = 0, hi = nt - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (item_start[mid] <= it) lo = mid; else hi = mid - 1;
        }
        const int64_t t = lo;
        const int4 bx = box[t];
        const unsigned long long k = it - item_start[t];
        const unsigned long long w = (unsigned long long)(bx.y - bx.x + 1);
        const int i = bx.x + (int)(k % w), j = bx.z + (int)(k / w);
        float a[3], b[3], c[3];
        load_tri(tri[t], a, b, c);
        const int area = projected_area_sign(a, b, c);
        const float px = col_coord(Q.mx, i, Q.dx), py = col_coord(Q.my, j, Q.dy);
        if (!column_inside(a, b, c, area, px, py)) continue;
        const uint32_t cidx = (uint32_t)i * (uint32_t)Q.ny + (uint32_t)j;
        if (PASS == 0) atomicAdd(&col[cidx], 1u);
        else zrec[atomicAdd(&col[cidx], 1u)] = z_cross(a, b, c, area, px, py);
    }
}

// ---- the volume -------------------------------------------------------------------------------------------------------------
struct VolArgs {
    float* values;
    float* colors;            // null: the volume has none
    const float* mesh_colors; // null: the mesh has none (colours are zero)
    const int32_t* idx;
    int nx, ny, nz, pitch, z0;
    float mx, my, mz, dx, dy, dz;
    float band;
    double stop2;             // (the band's f32 successor)^2: every d2 whose f32 distance is <= band lies below it
    const uint32_t* cstart;   // nx * ny + 1
    const double* zrec;
    const uint8_t* sign;      // null: parity of the crossings; else a byte per voxel (unpadded, z fastest), non-zero: inside
    unsigned long long* candidates;
};

__global__ __launch_bounds__(kBlock) void k_tm_volume(SearchGrid S, VolArgs A)
{
    const int64_t n = (int64_t)A.nx * A.ny * A.nz;
    const int64_t g0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool active = g0 < n;
    const int64_t gidx = active ? g0 : 0;
    const int k = (int)(gidx % A.nz);
    const int64_t row = gidx / A.nz;   // = i * ny + j
    const int j = (int)(row % A.ny), i = (int)(row / A.ny);
    const float q[3] = {col_coord(A.mx, i, A.dx), col_coord(A.my, j, A.dy), col_coord(A.mz, A.z0 + k, A.dz)};
    Best B;
    B.ncand = 0;
    B.bi = -1;
    if (active) tm_search(S, q, A.stop2, B);
    wave_add(A.candidates, B.ncand);
    if (!active) return;
    unsigned cnt = 0;
    if (A.sign) cnt = A.sign[g0] ? 1u : 0u;   // (the caller's sign: lib_trimesh_winding.hip)
    else {
        // parity of the crossings of this column below the voxel centre
        const double zk = (double)q[2];
        for (uint32_t r = A.cstart[row], r1 = A.cstart[row + 1]; r < r1; r++) cnt += A.zrec[r] < zk ? 1u : 0u;
    }
    float d = B.bi >= 0 ? (float)__builtin_sqrt(B.d2) : INFINITY;
    const bool clamped = d > A.band;   // (decided on the f32 distance: the same voxels as the +inf run's values say)
    if (clamped) d = A.band;
    const size_t o = (size_t)row * A.pitch + k;
    A.values[o] = (cnt & 1u) ? -d : d;
    if (A.colors) {
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        if (A.mesh_colors && !clamped) {
            const int32_t* t = A.idx + 3 * (int64_t)B.bi;
            const float* ca = A.mesh_colors + 3 * (int64_t)t[0];
            const float* cb = A.mesh_colors + 3 * (int64_t)t[1];
            const float* cc = A.mesh_colors + 3 * (int64_t)t[2];
            blend_colour(ca, cb, cc, B.cl.w, rgb);
        }
        for (int a = 0; a < 3; a++) A.colors[3 * o + a] = rgb[a];
    }
}

// ---- sampling ---------------------------------------------------------------------------------------------------------------
constexpr int kAreaParts = 1024;

// A2 per triangle and the per-block max -> part[block]; then one block -> part[kAreaParts] (a max is order-free)
__global__ __launch_bounds__(kBlock) void k_tm_area2(const TriPack* __restrict__ tri, int64_t nt, double* __restrict__ a2, double* __restrict__ part,
                                                     int final_pass)
{
    __shared__ double s[kBlock];
    double r = 0.0;
    if (!final_pass) {
        for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < nt; t += (int64_t)gridDim.x * kBlock) {
            float a[3], b[3], c[3];
            double n[3];
            load_tri(tri[t], a, b, c);
            const double v = smp::area2(a, b, c, n);
            a2[t] = v;
            r = fmax(r, v);
        }
    } else {
        for (int64_t b = threadIdx.x; b < nt; b += kBlock) r = fmax(r, part[b]);   // (nt = the number of partials here)
    }
    s[threadIdx.x] = r;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[final_pass ? kAreaParts : (int64_t)blockIdx.x] = s[0];
}

// the integer weights (0 everywhere when no triangle has an area) and the number of non-zero ones
__global__ __launch_bounds__(kBlock) void k_tm_sample_weights(const double* __restrict__ a2, int64_t nt, const double* __restrict__ a2max,
                                                              unsigned long long* __restrict__ w, unsigned long long* __restrict__ nonzero)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double m = *a2max;
    unsigned long long n = 0;
    if (t < nt) {
        const unsigned long long v = m > 0.0 ? smp::weight(a2[t], m) : 0ull;
        w[t] = v;
        n = v ? 1ull : 0ull;
    }
    n = wave_sum(n);   // (nonzero is never null)
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(nonzero, n);
}

struct SampleArgs {
    const TriPack* tri;
    const unsigned long long* W;   // nt + 1: W[nt] is the total, read here and not on the host
    int64_t nt;
    const int32_t* idx;
    const float* mesh_colors;      // null: the mesh has none (colours are zero)
    int64_t n;
    uint64_t seed;
    int stratified;
    float* points;
    float* normals;
    float* colors;
    int32_t* triangle;
    float* weights;
};

__global__ __launch_bounds__(kBlock) void k_tm_sample(SampleArgs A)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= A.n) return;
    const uint64_t total = A.W[A.nt];
    const uint64_t h0 = smp::draw(A.seed, (uint64_t)s, 0), h1 = smp::draw(A.seed, (uint64_t)s, 1), h2 = smp::draw(A.seed, (uint64_t)s, 2);
    const uint64_t r = smp::pick(h0, (uint64_t)s, (uint64_t)A.n, total, A.stratified != 0);
    const int64_t t = smp::find_triangle(A.W, A.nt, r);
    float a[3], b[3], c[3];
    load_tri(A.tri[t], a, b, c);
    const smp::Sample S = smp::sample_on(a, b, c, h1, h2);
    if (A.points)
        for (int k = 0; k < 3; k++) A.points[3 * s + k] = S.point[k];
    if (A.normals)
        for (int k = 0; k < 3; k++) A.normals[3 * s + k] = S.normal[k];
    if (A.colors) {
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        if (A.mesh_colors) {
            const int32_t* v = A.idx + 3 * t;
            smp::blend_colour(A.mesh_colors + 3 * (int64_t)v[0], A.mesh_colors + 3 * (int64_t)v[1], A.mesh_colors + 3 * (int64_t)v[2], S.w, rgb);
        }
        for (int k = 0; k < 3; k++) A.colors[3 * s + k] = rgb[k];
    }
    if (A.triangle) A.triangle[s] = (int32_t)t;
    if (A.weights)
        for (int k = 0; k < 3; k++) A.weights[3 * s + k] = S.weights[k];
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// the handle
// ---------------------------------------------------------------------------------------------------------------------------
// (struct sdfk_trimesh: trimesh_handle.h)
// The sampling weights and their scan, once per handle: synchronises to read the total (trimesh_handle.h).
int trimesh_weights(sdfk_trimesh* t, const char* who)
{
    if (t->sample_W) return SDFK_OK;
    const int64_t nt = t->nt;
    const unsigned bb = (unsigned)std::min<int64_t>(kAreaParts, (nt + kBlock - 1) / kBlock);
    Staged st;
    unsigned long long* W = st.kept<unsigned long long>((size_t)nt + 1);
    double* a2 = st.scratch<double>((size_t)nt);
    double* part = st.scratch<double>(kAreaParts + 1);
    unsigned long long* nonzero = st.scratch<unsigned long long>(1);
    struct { double a2max; unsigned long long nonzero, total; } host{};
    st.run([&] { return hipMemsetAsync(nonzero, 0, sizeof(unsigned long long), g.stream); });
    st.run([&] {
        {
            ProfScope ps("k_tm_area2");
            hipLaunchKernelGGL(k_tm_area2, dim3(bb), dim3(kBlock), 0, g.stream, t->tri, nt, a2, part, 0);
            hipLaunchKernelGGL(k_tm_area2, dim3(1), dim3(kBlock), 0, g.stream, t->tri, (int64_t)bb, a2, part, 1);
        }
        ProfScope ps("k_tm_sample_weights");
        hipLaunchKernelGGL(k_tm_sample_weights, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, a2, nt, part + kAreaParts, W, nonzero);
    });
    st.run([&] { return sdfk_scan::scan(W, nt, who); });
    st.run([&] { return hipMemcpyAsync(&host.a2max, part + kAreaParts, sizeof(double), hipMemcpyDeviceToHost, g.stream); });
    st.run([&] { return hipMemcpyAsync(&host.nonzero, nonzero, sizeof(unsigned long long), hipMemcpyDeviceToHost, g.stream); });
    st.read(&host.total, W + nt, sizeof host.total);
    if (int r = st.finish(who, false)) return r;
    t->sample_W = W;
    t->sample_no_area = !(host.a2max > 0.0);
    t->sample_nonzero = (int64_t)host.nonzero;
    t->sample_total = (int64_t)host.total;
    return SDFK_OK;
}

// What every entry point of the family asks of its handle first (trimesh_handle.h).
int trimesh_check(const sdfk_trimesh* t, const char* who, int records)
{
    if (int r = require_init()) return r;
    if (!t) return fail(SDFK_ERR_INVALID, "%s: null argument", who);
    if (records && records * t->nt >= (int64_t(1) << 32)) return fail(SDFK_ERR_INVALID, "%s: 2^32 / %d triangles or more", who, records);
    return SDFK_OK;
}

namespace {

void trimesh_release(sdfk_trimesh* t)
{
    dev_free(t->vertices); dev_free(t->colors); dev_free(t->idx); dev_free(t->tri);
    dev_free(t->list); dev_free(t->starts); dev_free(t->ystarts); dev_free(t->sample_W);
    dev_free(t->comp_vertex); dev_free(t->comp_triangle);
    dev_free(t->nbr_start); dev_free(t->nbr); dev_free(t->boundary); dev_free(t->inc_start); dev_free(t->inc);
    dev_free(t->wn_nodes); dev_free(t->wn_order);
    t->wn_nodes = nullptr; t->wn_order = nullptr;
    t->sample_W = nullptr;
    t->comp_vertex = t->comp_triangle = nullptr;
    t->nbr_start = t->nbr = t->inc_start = t->inc = nullptr; t->boundary = nullptr;
    t->vertices = t->colors = nullptr; t->idx = nullptr; t->tri = nullptr; t->list = t->starts = t->ystarts = nullptr;
}

SearchGrid search_grid(const sdfk_trimesh* t) { return SearchGrid{t->tri, t->list, t->starts, t->ystarts, t->G}; }

int trimesh_build(sdfk_trimesh* t)
{
    static const char* who = "sdfk_trimesh_create";
    const int64_t nt = t->nt;
    const unsigned bb = (unsigned)std::min<int64_t>(1024, (nt + kBlock - 1) / kBlock);
    struct { unsigned flags[4]; float box[8]; } host{};
    // (tri, starts, list and ystarts are the handle's from the start: trimesh_make releases them with it when this fails)
    Staged st;
    st.run([&] { return dev_alloc((void**)&t->tri, (size_t)nt * sizeof(TriPack)); });
    unsigned* flags = st.scratch<unsigned>(4);
    float* part = st.scratch<float>((1024 + 1) * 8);
    {
        ProfScope ps("k_tm_pack");
        st.run([&] { return hipMemsetAsync(flags, 0, 4 * sizeof(unsigned), g.stream); });
        st.run([&] {
            hipLaunchKernelGGL(k_tm_vcheck, dim3(grid1(std::min<int64_t>(3 * t->nv, int64_t(1) << 20))), dim3(kBlock), 0, g.stream, t->vertices, t->nv, flags);
            hipLaunchKernelGGL(k_tm_pack, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->vertices, t->nv, t->idx, nt, t->tri, flags);
            hipLaunchKernelGGL(k_tm_bounds, dim3(bb), dim3(kBlock), 0, g.stream, t->tri, nt, part, 0);
            hipLaunchKernelGGL(k_tm_bounds, dim3(1), dim3(kBlock), 0, g.stream, t->tri, (int64_t)bb, part, 1);
        });
        st.run([&] { return hipMemcpyAsync(host.flags, flags, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, g.stream); });
        st.read(host.box, part + 8 * 1024, 6 * sizeof(float));
    }
    if (int r = st.finish(who, false)) return r;
    if (host.flags[0]) return fail(SDFK_ERR_INVALID, "%s: a triangle index is outside [0, n_vertices)", who);
    if (host.flags[1]) return fail(SDFK_ERR_INVALID, "%s: a vertex has a NaN or infinite coordinate", who);

    t->G = grid_for_box(host.box, host.box + 3, nt);
    t->cells = (int64_t)t->G.dim[0] * t->G.dim[1] * t->G.dim[2];
    unsigned long long entries = 0;
    st.run([&] { return dev_alloc((void**)&t->starts, (size_t)(t->cells + 1) * sizeof(uint32_t)); });
    unsigned long long* total = st.scratch<unsigned long long>(1);
    {
        ProfScope ps("k_tm_bin");
        st.run([&] { return hipMemsetAsync(t->starts, 0, (size_t)(t->cells + 1) * sizeof(uint32_t), g.stream); });
        st.run([&] { return hipMemsetAsync(total, 0, sizeof(unsigned long long), g.stream); });
        st.run([&] { hipLaunchKernelGGL(k_tm_bin_count, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->tri, nt, t->G, t->starts, total); });
        st.read(&entries, total, sizeof entries);
    }
    if (int r = st.finish(who, false)) return r;
    if (entries >= (1ull << 32)) return fail(SDFK_ERR_INVALID, "%s: 2^32 triangle-cell pairs or more", who);
    t->entries = (int64_t)entries;
    st.run([&] { return sdfk_scan::scan(t->starts, t->cells, who); });
    st.run([&] { return dev_alloc((void**)&t->list, (size_t)std::max<int64_t>(t->entries, 1) * sizeof(uint32_t)); });
    uint32_t* cursor = st.scratch<uint32_t>((size_t)t->cells);
    st.run([&] { return dev_alloc((void**)&t->ystarts, (size_t)(t->cells + 1) * sizeof(uint32_t)); });
    {
        ProfScope ps("k_tm_bin");
        st.run([&] { return hipMemcpyAsync(cursor, t->starts, (size_t)t->cells * sizeof(uint32_t), hipMemcpyDeviceToDevice, g.stream); });
        st.run([&] {
            hipLaunchKernelGGL(k_tm_bin_scatter, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->tri, nt, t->G, cursor, t->list);
            hipLaunchKernelGGL(k_tm_ycounts, dim3(grid1(t->cells)), dim3(kBlock), 0, g.stream, t->starts, t->G, t->cells, t->ystarts);
        });
    }
    st.run([&] { return sdfk_scan::scan(t->ystarts, t->cells, who); });
    return st.finish(who);   // (synchronises: the caller's arrays are not retained)
}

int trimesh_make(const void* v, int64_t nv, const void* tris, int64_t ni, const void* colors, bool device, sdfk_trimesh** out)
{
    static const char* who = "sdfk_trimesh_create";
    if (int r = require_init()) return r;
    if (!out) return fail(SDFK_ERR_INVALID, "%s: null argument", who);
    *out = nullptr;
    if (ni < 3 || ni % 3 != 0) return fail(SDFK_ERR_INVALID, "%s: n_indices must be a positive multiple of 3", who);
    if (ni / 3 >= (int64_t(1) << 31)) return fail(SDFK_ERR_INVALID, "%s: 2^31 triangles or more", who);
    if (nv < 1 || nv >= (int64_t(1) << 31)) return fail(SDFK_ERR_INVALID, "%s: n_vertices must be in [1, 2^31)", who);
    if (!v || !tris) return fail(SDFK_ERR_INVALID, "%s: null vertices / triangles", who);
    sdfk_trimesh* t = new sdfk_trimesh();
    t->nv = nv;
    t->nt = ni / 3;
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    // (written out, not Staged: there is no scratch here -- the three arrays are the handle's at once, and trimesh_release frees them)
    int r = dev_alloc((void**)&t->vertices, (size_t)nv * 3 * sizeof(float));
    if (!r) r = dev_alloc((void**)&t->idx, (size_t)ni * sizeof(int32_t));
    if (!r && colors) r = dev_alloc((void**)&t->colors, (size_t)nv * 3 * sizeof(float));
    if (!r) {
        hipError_t e = hipMemcpyAsync(t->vertices, v, (size_t)nv * 3 * sizeof(float), kind, g.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(t->idx, tris, (size_t)ni * sizeof(int32_t), kind, g.stream);
        if (e == hipSuccess && colors) e = hipMemcpyAsync(t->colors, colors, (size_t)nv * 3 * sizeof(float), kind, g.stream);
        if (e != hipSuccess) r = fail(SDFK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    if (!r) r = trimesh_build(t);   // (synchronises)
    if (r) {
        trimesh_release(t);
        delete t;
        return r;
    }
    *out = t;
    return SDFK_OK;
}

int closest_launch(const sdfk_trimesh* t, const float* q, int64_t n, QueryOut O)
{
    Staged st;
    ProfCount<1> pc;
    pc.begin(st);
    O.candidates = pc.dev;
    st.run([&] {
        ProfScope ps("k_tm_closest");
        hipLaunchKernelGGL(k_tm_closest, dim3(grid1(n)), dim3(kBlock), 0, g.stream, search_grid(t), q, n, O);
    });
    trimesh_keep_count(st, pc, t, n);
    return st.finish("sdfk_trimesh_closest", false);
}

int to_volume(const sdfk_trimesh* t, sdfk_volume* v, float band, const uint8_t* sign)
{
    static const char* who = "sdfk_trimesh_to_volume";
    if (v->elided || !v->values) return fail(SDFK_ERR_INVALID, "%s: the volume has no storage", who);
    resolve_dependents(v);   // (a queued mesh may still read the old values)
    volume_values_changed(v);
    float d[3], m[3], outside;
    grid_constants(v, d, m, &outside);
    const Columns Q{v->nx, v->ny, m[0], m[1], d[0], d[1]};
    const int64_t nt = t->nt, ncol = (int64_t)v->nx * v->ny;
    Staged st;
    uint32_t* col = nullptr;
    double* zrec = nullptr;
    unsigned long long n_items = 0;
    uint32_t n_cross = 0;
    auto grid_items = [](unsigned long long n) { return (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>((n + kBlock - 1) / kBlock, 1u << 20)); };
    if (!sign) {
        int4* box = st.scratch<int4>((size_t)nt);
        unsigned long long* items = st.scratch<unsigned long long>((size_t)nt + 1);
        col = st.scratch<uint32_t>((size_t)ncol + 1);
        uint32_t* cursor = st.scratch<uint32_t>((size_t)ncol);
        ProfScope ps("k_tm_cross");
        st.run([&] { hipLaunchKernelGGL(k_tm_items, dim3(grid1(nt)), dim3(kBlock), 0, g.stream, t->tri, nt, Q, box, items); });
        st.run([&] { return sdfk_scan::scan(items, nt, who); });
        st.run([&] { return hipMemsetAsync(col, 0, (size_t)(ncol + 1) * sizeof(uint32_t), g.stream); });
        st.read(&n_items, items + nt, sizeof n_items);
        if (n_items)
            st.run([&] {
                hipLaunchKernelGGL(k_tm_cross<0>, dim3(grid_items(n_items)), dim3(kBlock), 0, g.stream, t->tri, nt, Q, box, items, n_items, col, nullptr);
            });
        st.run([&] { return sdfk_scan::scan(col, ncol, who); });
        st.read(&n_cross, col + ncol, sizeof n_cross);
        zrec = st.scratch<double>(std::max<uint32_t>(n_cross, 1));
        st.run([&] { return hipMemcpyAsync(cursor, col, (size_t)ncol * sizeof(uint32_t), hipMemcpyDeviceToDevice, g.stream); });
        if (n_cross)
            st.run([&] {
                hipLaunchKernelGGL(k_tm_cross<1>, dim3(grid_items(n_items)), dim3(kBlock), 0, g.stream, t->tri, nt, Q, box, items, n_items, cursor, zrec);
            });
    }
    ProfCount<1> pc;
    pc.begin(st);
    // every d2 whose f32 distance (float)sqrt(d2) is <= band is below next^2 (next: the f32 after band), so the search may stop
    // there: a voxel it leaves unresolved has an f32 distance > band and is clamped, as its exact distance would be
    const double next = (double)nextafterf(band, INFINITY);
    const double stop2 = next * next;
    st.run([&] {
        VolArgs A{v->values, v->colors, t->colors, t->idx, v->nx, v->ny, v->nz, v->pitch(), v->z0, m[0], m[1], m[2], d[0], d[1], d[2],
                  band, stop2, col, zrec, sign, pc.dev};
        ProfScope ps("k_tm_volume");
        hipLaunchKernelGGL(k_tm_volume, dim3(grid1((int64_t)v->nx * v->ny * v->nz)), dim3(kBlock), 0, g.stream, search_grid(t), A);
    });
    trimesh_keep_count(st, pc, t, (int64_t)v->nx * v->ny * v->nz);
    const_cast<sdfk_trimesh*>(t)->last_crossings = n_cross;
    return st.finish(who, false);   // (on success the scratch goes back to the stream-ordered pool under the queued volume pass)
}

// the weights, and the sampler's refusal of a mesh without area
int sample_prepare(sdfk_trimesh* t, const char* who)
{
    if (int r = trimesh_weights(t, who)) return r;
    if (t->sample_no_area) return fail(SDFK_ERR_INVALID, "%s: no triangle has an area", who);
    return SDFK_OK;
}

int sample_check(const sdfk_trimesh* t, int64_t n, int32_t flags, const char* who)
{
    if (int r = trimesh_check(t, who, 0)) return r;
    if (n < 0 || n >= (int64_t(1) << 31)) return fail(SDFK_ERR_INVALID, "%s: n must be in [0, 2^31)", who);
    if (flags & ~SDFK_TRIMESH_SAMPLE_STRATIFIED) return fail(SDFK_ERR_INVALID, "%s: unknown flag bits", who);
    return SDFK_OK;
}

int sample_launch(const sdfk_trimesh* t, int64_t n, uint64_t seed, int32_t flags, float* points, float* normals, float* colors, int32_t* triangle,
                  float* weights, const char* who)
{
    const SampleArgs A{t->tri, t->sample_W, t->nt, t->idx, t->colors, n, seed, flags & SDFK_TRIMESH_SAMPLE_STRATIFIED, points, normals, colors,
                       triangle, weights};
    {
        ProfScope ps("k_tm_sample");
        hipLaunchKernelGGL(k_tm_sample, dim3(grid1(n)), dim3(kBlock), 0, g.stream, A);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SDFK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return SDFK_OK;
}

void sample_stats(const sdfk_trimesh* t, int64_t stats[2])
{
    if (!stats) return;
    stats[0] = t->sample_nonzero;
    stats[1] = t->sample_total;
}

}  // namespace

int trimesh_to_volume(const sdfk_trimesh* t, sdfk_volume* v, float band, const uint8_t* sign_dev) { return to_volume(t, v, band, sign_dev); }

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_trimesh_create(const float* vertices3, int64_t n_vertices, const int32_t* triangles, int64_t n_indices, const float* colors3,
                                   sdfk_trimesh** out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return trimesh_make(vertices3, n_vertices, triangles, n_indices, colors3, false, out);
}

extern "C" int sdfk_trimesh_create_device(const void* vertices3_dev, int64_t n_vertices, const void* triangles_dev, int64_t n_indices,
                                          const void* colors3_dev, sdfk_trimesh** out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return trimesh_make(vertices3_dev, n_vertices, triangles_dev, n_indices, colors3_dev, true, out);
}

extern "C" int sdfk_trimesh_closest_device(const sdfk_trimesh* t, const void* queries3_dev, int64_t n, void* triangle_dev, void* distance_dev,
                                           void* closest3_dev)
{
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = require_init()) return r;
    if (!t || n < 0 || (n > 0 && !queries3_dev)) return fail(SDFK_ERR_INVALID, "sdfk_trimesh_closest: null / negative argument");
    if (n >= (int64_t(1) << 32)) return fail(SDFK_ERR_INVALID, "sdfk_trimesh_closest: 2^32 queries or more");
    if (n == 0) return SDFK_OK;
    return closest_launch(t, (const float*)queries3_dev, n, QueryOut{(int32_t*)triangle_dev, (float*)distance_dev, (float*)closest3_dev, nullptr});
}

extern "C" int sdfk_trimesh_closest(const sdfk_trimesh* t, const float* queries3, int64_t n, int32_t* triangle, float* distance, float* closest3)
{
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = require_init()) return r;
    if (!t || n < 0 || (n > 0 && !queries3)) return fail(SDFK_ERR_INVALID, "sdfk_trimesh_closest: null / negative argument");
    if (n >= (int64_t(1) << 32)) return fail(SDFK_ERR_INVALID, "sdfk_trimesh_closest: 2^32 queries or more");
    if (n == 0) return SDFK_OK;
    Staged st;
    const float* qd = st.in(queries3, (size_t)n * 3);
    const QueryOut O{st.out(triangle, (size_t)n), st.out(distance, (size_t)n), st.out(closest3, (size_t)n * 3), nullptr};
    st.run([&] { return closest_launch(t, qd, n, O); });
    return st.finish("sdfk_trimesh_closest");
}

extern "C" int sdfk_trimesh_to_volume(const sdfk_trimesh* t, sdfk_volume* v, float max_distance)
{
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = require_init()) return r;
    if (!t || !v) return fail(SDFK_ERR_INVALID, "sdfk_trimesh_to_volume: null argument");
    if (!(max_distance >= 0.0f)) return fail(SDFK_ERR_INVALID, "sdfk_trimesh_to_volume: max_distance must be >= 0 (+inf: exact everywhere)");
    return to_volume(t, v, max_distance, nullptr);
}

extern "C" int sdfk_trimesh_sample_device(sdfk_trimesh* t, int64_t n, uint64_t seed, int32_t flags, void* points3_dev, void* normals3_dev,
                                          void* colors3_dev, void* triangle_dev, void* weights3_dev, int64_t stats[2])
{
    static const char* who = "sdfk_trimesh_sample";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = sample_check(t, n, flags, who)) return r;
    if (n == 0) return SDFK_OK;
    if (int r = sample_prepare(t, who)) return r;
    sample_stats(t, stats);
    return sample_launch(t, n, seed, flags, (float*)points3_dev, (float*)normals3_dev, (float*)colors3_dev, (int32_t*)triangle_dev,
                         (float*)weights3_dev, who);
}

extern "C" int sdfk_trimesh_sample(sdfk_trimesh* t, int64_t n, uint64_t seed, int32_t flags, float* points3, float* normals3, float* colors3,
                                   int32_t* triangle, float* weights3, int64_t stats[2])
{
    static const char* who = "sdfk_trimesh_sample";
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = sample_check(t, n, flags, who)) return r;
    if (n == 0) return SDFK_OK;
    if (int r = sample_prepare(t, who)) return r;
    sample_stats(t, stats);
    const size_t n3 = (size_t)n * 3;
    Staged st;
    float* pd = st.out(points3, n3);
    float* nd = st.out(normals3, n3);
    float* cd = st.out(colors3, n3);
    int32_t* td = st.out(triangle, (size_t)n);
    float* wd = st.out(weights3, n3);
    st.run([&] { return sample_launch(t, n, seed, flags, pd, nd, cd, td, wd, who); });
    return st.finish(who);
}

extern "C" int sdfk_trimesh_stats(const sdfk_trimesh* t, int64_t stats[8])
{
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!t || !stats) return fail(SDFK_ERR_INVALID, "sdfk_trimesh_stats: null argument");
    stats[0] = t->G.dim[0];
    stats[1] = t->G.dim[1];
    stats[2] = t->G.dim[2];
    stats[3] = t->nt;
    stats[4] = t->entries;
    stats[5] = t->last_candidates;
    stats[6] = t->last_queries;
    stats[7] = t->last_crossings;
    return SDFK_OK;
}

extern "C" void sdfk_trimesh_free(sdfk_trimesh* t)
{
    StateScope in_owner_context(t ? t->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    bind_thread();
    if (!t) return;
    if (g.inited) trimesh_release(t);
    delete t;
}
