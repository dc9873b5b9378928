// lib_points.hip -- KdTree (KdTree.cs) and IterativeClosestPoint (IterativeClosestPoint.cs): exact nearest-point search against a
// static point set, and rigid ICP registration built on it.  Contract: include/sdfkit_hip.h, "KdTree / IterativeClosestPoint".
//
// Search structure: a uniform grid of sorted cell lists, built on the device by a counting sort --
//   bounds (+ the non-finite check) -> cell key per point and per-cell counts (integer atomics) -> exclusive scan -> scatter into
//   float4 (x, y, z, bits(index)) in cell order, so that one 16-byte load gives a candidate.
// In-cell order comes from the atomics and varies from build to build; the (d2, index) rule makes every result independent of it.
// Query: one lane per query on the shell walk that every query of the KdTree runs (points_walk.h, walk_launch): cells in growing
// Chebyshev shells around the query's cell (clamped to the grid); k_pts_search's visitor keeps the least (d2, index) and stops
// the walk when the conservative f32 lower bound on the d2 of every unvisited cell exceeds it.  Queries run in the caller's order:
// processing them in the order of a coarse counting sort of their cells was measured slower for mesh vertices, whose order is
// already spatially coherent, and 5 % faster only for random queries (profiles/points_ab_query_order.txt).  Grid sizing and cell
// assignment: points_grid.h.
// ICP: per iteration search -> sum of d, then of (d - mean)^2 -> filtered sums (count, p, q) -> centred C -> a one-lane solve (f64 SVD, the
// reference's f32 Matrix4x4 steps, convergence, running total) -> the step applied to the points.  Every reduction is f64 in the
// fixed order of device_reduce.h (per-block partials of its fixed grid, then one block), with no float atomics: results are bitwise
// reproducible.
// Everything after the reductions (the distMax rule, the filter, the solve, the Matrix4x4 steps) is icp_solve.h, shared with the host.
// With a normal per static point the same loop runs the point-to-plane metric: kept count and mean -> the 28 sums of the 6x6 normal
// equations -> a one-lane eigen-solve and Cayley step ("ICP, point to plane" below).
// Host side: the scratch of the build and of the ICP, and the arrays a build makes for the handle (kept until it succeeded), are
// held in a Staged (device_stage.h); points_release alone frees what a handle owns.
#include "lib_internal.h"
#include "device_reduce.h"
#include "device_scan.h"
#include "points_grid.h"
#include "points_set.h"
#include "points_walk.h"
#include "icp_solve.h"

#include <cfloat>

namespace {

using namespace sdfk_points_grid;   // Grid, cell_of, key_of, grid_for_box; kMaxCells, kMaxAxisCells
using sdfk_walk::grid_of;
using sdfk_walk::kBlock;
using namespace sdfk_reduce;        // the fixed-order reductions of the ICP, both levels
static_assert(kBlock == kReduceBlock, "the reductions run in blocks of device_reduce.h's size");

// ---- build ------------------------------------------------------------------------------------------------------------------
// the box so far and another: least of the three minima, greatest of the three maxima and of the non-finite count or flag
__device__ __forceinline__ void bounds_merge(float* r, const float* o, int stride)
{
    for (int j = 0; j < 3; j++) r[j * stride] = fminf(r[j * stride], o[j * stride]);
    for (int j = 3; j < 7; j++) r[j * stride] = fmaxf(r[j * stride], o[j * stride]);   // (any non-finite point: > 0)
}

// the block's box of its threads' boxes -> s[0 .. 6][0]
__device__ __forceinline__ void bounds_tree(const float (&r)[7], float (*s)[kBlock])
{
    for (int j = 0; j < 7; j++) s[j][threadIdx.x] = r[j];
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) bounds_merge(&s[0][threadIdx.x], &s[0][threadIdx.x + o], kBlock);
        __syncthreads();
    }
}

// per-block min / max of each coordinate and the number of non-finite points -> part[block][8]
__global__ __launch_bounds__(kBlock) void k_pts_bounds(const float* __restrict__ p, int64_t n, float* __restrict__ part)
{
    __shared__ float s[7][kBlock];
    float r[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0f};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) { r[6] += 1.0f; continue; }
        r[0] = fminf(r[0], x); r[1] = fminf(r[1], y); r[2] = fminf(r[2], z);
        r[3] = fmaxf(r[3], x); r[4] = fmaxf(r[4], y); r[5] = fmaxf(r[5], z);
    }
    bounds_tree(r, s);
    if (threadIdx.x < 7) part[blockIdx.x * 8 + threadIdx.x] = s[threadIdx.x][0];
}

__global__ __launch_bounds__(kBlock) void k_pts_bounds_final(const float* __restrict__ part, int blocks, float* __restrict__ out)
{
    __shared__ float s[7][kBlock];
    float r[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0f};
    for (int b = threadIdx.x; b < blocks; b += kBlock) bounds_merge(r, part + b * 8, 1);
    bounds_tree(r, s);
    if (threadIdx.x < 7) out[threadIdx.x] = s[threadIdx.x][0];
}

__global__ __launch_bounds__(kBlock) void k_pts_count(const float* __restrict__ p, int64_t n, Grid G, uint32_t* __restrict__ keys,
                                                      uint32_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int cx, cy, cz;
    const uint32_t k = key_of(G, p[3 * i], p[3 * i + 1], p[3 * i + 2], &cx, &cy, &cz);
    keys[i] = k;
    atomicAdd(&counts[k], 1u);
}

// the exclusive scan of the cell counts: device_scan.h

__global__ __launch_bounds__(kBlock) void k_pts_scatter(const float* __restrict__ p, int64_t n, const uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ cursor, float4* __restrict__ sorted)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = atomicAdd(&cursor[keys[i]], 1u);
    sorted[slot] = make_float4(p[3 * i], p[3 * i + 1], p[3 * i + 2], __int_as_float((int)i));
}

// ---- query ------------------------------------------------------------------------------------------------------------------
struct SearchOut {
    int32_t* index;     // any may be null
    float* distance;
    float* nearest3;
    float4* cor;        // ICP: (x, y, z, distance) of the nearest point, caller order
    unsigned long long* candidates;   // non-null: count candidates (measurement)
};

struct IcpState;
__device__ __forceinline__ bool icp_stopped(const IcpState* S, int iter);

// what the walk keeps for the nearest point: the least (d2, index) and that point's coordinates
struct NearestVisitor {
    float best;
    int bi;
    float bx, by, bz;
    __device__ __forceinline__ void take(float d2, const float4& s)
    {
        const int id = __float_as_int(s.w);
        if (d2 < best || (d2 == best && id < bi)) { best = d2; bi = id; bx = s.x; by = s.y; bz = s.z; }
    }
    // (the FLT_MAX bound is the k-nearest rule's for "no radius", points_knn.h walk_done: a point counts iff d2 < +inf, so once the
    // lower bound of every unvisited cell is +inf nothing that is left can be taken, found or not)
    __device__ __forceinline__ bool done(float lb2) const { return lb2 * (1.0f - 0x1p-18f) > fminf(best, FLT_MAX); }
};

// One lane per query.  `icp` / `iter`: ICP iterations exit once the registration stopped.  A query without a nearest point
// (non-finite, or every d2 overflows) gets index -1, distance FLT_MAX and the first static point (fx, fy, fz).
__global__ __launch_bounds__(kBlock) void k_pts_search(const float4* __restrict__ sorted, const uint32_t* __restrict__ starts, Grid G,
                                                       float fx, float fy, float fz, const float* __restrict__ queries, int64_t nq,
                                                       SearchOut O, const IcpState* icp, int iter)
{
    if (icp && icp_stopped(icp, iter)) return;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const sdfk_walk::Query q = sdfk_walk::load_query(queries, t, nq);
    NearestVisitor v{INFINITY, -1, fx, fy, fz};
    unsigned long long ncand = 0;
    if (q.finite) ncand = sdfk_walk::shell_walk(sorted, starts, G, q.x, q.y, q.z, v);
    const float dist = v.bi < 0 ? FLT_MAX : (float)__builtin_sqrt((double)v.best);   // (correctly rounded sqrtf)
    wave_add(O.candidates, ncand);   // (every lane stays for the shuffle)
    if (t >= nq) return;
    if (O.index) O.index[t] = v.bi;
    if (O.distance) O.distance[t] = dist;
    if (O.nearest3) { O.nearest3[3 * t] = v.bx; O.nearest3[3 * t + 1] = v.by; O.nearest3[3 * t + 2] = v.bz; }
    if (O.cor) O.cor[t] = make_float4(v.bx, v.by, v.bz, dist);
}

// ---- ICP --------------------------------------------------------------------------------------------------------------------
struct IcpState {
    double part[kReduceBlocks][9];   // per-block partial sums of the current reduction
    double dist_mean;             // this iteration's distance mean (f64)
    float dist_max;               // this iteration's filter
    double pmean[3], qmean[3];    // filtered means (f64)
    float step[16], total[16];    // row-major M11..M44
    int iters;                    // iterations completed
    int stop;                     // converged or max_iterations reached
    int converged;
};

__device__ __forceinline__ bool icp_stopped(const IcpState* S, int iter) { return S->stop && S->iters <= iter; }

struct IcpArgs {
    float* points;        // n x 3, moved in place
    const float4* cor;    // nearest static point + distance per point
    int64_t n;
    float good, conv_t, conv_r;
    int max_iters;
    IcpState* S;
};

// pass 1: sum d -> part[b][0]
__global__ __launch_bounds__(kBlock) void k_icp_dsum(IcpArgs A, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[1][kBlock];
    double v[1];
    grid_sum(A.n, v, s, [&](int64_t i, double* acc) { acc[0] += A.cor[i].w; });
    if (threadIdx.x == 0) A.S->part[blockIdx.x][0] = v[0];
}

// pass 2: the mean (every block reduces pass 1's partials alike), then sum (d - mean)^2 -> part[b][1], the reference's
// two-pass form (IterativeClosestPoint.cs:95-100)
__global__ __launch_bounds__(kBlock) void k_icp_dvar(IcpArgs A, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[1][kBlock];
    double m[1];
    sum_partials(A.S->part, 0, m, s);
    const double mean = m[0] / (double)A.n;
    __syncthreads();   // (s is reused)
    double v[1];
    grid_sum(A.n, v, s, [&](int64_t i, double* acc) {
        const double d = (double)A.cor[i].w - mean;
        acc[0] += d * d;
    });
    if (threadIdx.x == 0) {
        A.S->part[blockIdx.x][1] = v[0];
        if (blockIdx.x == 0) A.S->dist_mean = mean;
    }
}

__global__ __launch_bounds__(kBlock) void k_icp_dstats(IcpArgs A, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[1][kBlock];
    double r[1];
    sum_partials(A.S->part, 1, r, s);
    if (threadIdx.x != 0) return;
    A.S->dist_max = sdfk_icp::dist_max(A.S->dist_mean, r[0], (double)A.n, A.good);   // (icp_solve.h)
}

// pass 2: count, sum p, sum q of the points with dist <= distMax
__global__ __launch_bounds__(kBlock) void k_icp_fsum(IcpArgs A, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[7][kBlock];
    const float dmax = A.S->dist_max;
    double v[7];
    grid_sum(A.n, v, s, [&](int64_t i, double* acc) {
        const float4 c = A.cor[i];
        if (sdfk_icp::kept(c.w, dmax)) {
            acc[0] += 1.0;
            acc[1] += A.points[3 * i]; acc[2] += A.points[3 * i + 1]; acc[3] += A.points[3 * i + 2];
            acc[4] += c.x; acc[5] += c.y; acc[6] += c.z;
        }
    });
    if (threadIdx.x == 0)
        for (int j = 0; j < 7; j++) A.S->part[blockIdx.x][j] = v[j];
}

__global__ __launch_bounds__(kBlock) void k_icp_means(IcpArgs A, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[7][kBlock];
    double r[7];
    sum_partials(A.S->part, 0, r, s);
    if (threadIdx.x != 0) return;
    for (int j = 0; j < 3; j++) { A.S->pmean[j] = r[1 + j] / r[0]; A.S->qmean[j] = r[4 + j] / r[0]; }
}

// pass 3: C = sum (p - pmean)(q - qmean)^T over the filtered points
__global__ __launch_bounds__(kBlock) void k_icp_csum(IcpArgs A, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[9][kBlock];
    const float dmax = A.S->dist_max;
    const double pm0 = A.S->pmean[0], pm1 = A.S->pmean[1], pm2 = A.S->pmean[2];
    const double qm0 = A.S->qmean[0], qm1 = A.S->qmean[1], qm2 = A.S->qmean[2];
    double v[9];
    grid_sum(A.n, v, s, [&](int64_t i, double* acc) {
        const float4 c = A.cor[i];
        if (sdfk_icp::kept(c.w, dmax)) {
            const double p[3] = {A.points[3 * i] - pm0, A.points[3 * i + 1] - pm1, A.points[3 * i + 2] - pm2};
            const double q[3] = {c.x - qm0, c.y - qm1, c.z - qm2};
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) acc[3 * a + b] += p[a] * q[b];
        }
    });
    if (threadIdx.x == 0)
        for (int j = 0; j < 9; j++) A.S->part[blockIdx.x][j] = v[j];
}

// the solve (icp_solve.h) on one lane: the f64 SVD, the reference's f32 Matrix4x4 steps, convergence, the running total
__global__ __launch_bounds__(kBlock) void k_icp_solve(IcpArgs A, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[9][kBlock];
    double Cs[9];
    sum_partials(A.S->part, 0, Cs, s);
    if (threadIdx.x != 0) return;
    IcpState* S = A.S;
    float step[16], tot[16];
    bool conv;
    sdfk_icp::solve_step(Cs, S->pmean, S->qmean, S->total, A.conv_t, A.conv_r, step, tot, &conv);
    for (int q = 0; q < 16; q++) { S->step[q] = step[q]; S->total[q] = tot[q]; }
    S->iters = iter + 1;
    S->converged = conv;
    S->stop = conv || iter + 1 >= A.max_iters;
}

__global__ __launch_bounds__(kBlock) void k_icp_apply(IcpArgs A, int iter)
{
    if (icp_stopped(A.S, iter)) return;   // (the iteration that stopped the registration still moves the points)
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n) return;
    const float* m = A.S->step;
    const float x = A.points[3 * i], y = A.points[3 * i + 1], z = A.points[3 * i + 2];
    float o[3];
    for (int j = 0; j < 3; j++)
        o[j] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, m[j]), __fmul_rn(y, m[4 + j])), __fmul_rn(z, m[8 + j])), m[12 + j]);
    A.points[3 * i] = o[0]; A.points[3 * i + 1] = o[1]; A.points[3 * i + 2] = o[2];
}

__global__ void k_icp_init(IcpState* S)
{
    if (threadIdx.x != 0) return;
    for (int q = 0; q < 16; q++) { S->total[q] = (q % 5 == 0) ? 1.0f : 0.0f; S->step[q] = S->total[q]; }
    S->iters = 0;
    S->stop = 0;
    S->converged = 0;
}

// ---- ICP, point to plane ----------------------------------------------------------------------------------------------------
// The second metric: after the same search (which also delivers the static index) and distance statistics, the kept points' count
// and mean, then the 28 sums of the normal equations -- the 21 products J_a J_b (a <= b), the 6 products J_a r, and r r -- and a
// one-lane solve (icp_solve.h: plane_row, solve_step_plane).  A block reduces its 28 columns seven at a time through one [7][256]
// buffer (14 KB, the size k_icp_fsum uses): block_sum<28> would take 56 KB of the 160 KB LDS of a CU and leave room for two blocks
// where the accumulation loop, which is what takes the time, wants the CU full; the four passes cost 4 x 8 barriers per block.
constexpr int kPlaneCols = 28;
constexpr int kPlaneGroup = 7;

struct IcpPlane {
    double part[kReduceBlocks][kPlaneCols];   // per-block partial sums of the current reduction
    double count;                          // kept points of this iteration
    double rsq;                            // sum of r^2 over them, before the step
    int retained;                          // eigenvalues the solve retained
};

struct IcpPlaneArgs {
    const int32_t* index;    // the nearest static point per point (-1: none)
    const float* normals;    // one per static point
    IcpPlane* P;
};

// the correspondence of point i: whether it is kept, its static point and normal
__device__ __forceinline__ bool plane_cor(const IcpArgs& A, const IcpPlaneArgs& B, int64_t i, float dmax, float q[3], float nrm[3])
{
    const float4 c = A.cor[i];
    const int id = B.index[i];
    q[0] = c.x; q[1] = c.y; q[2] = c.z;
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
    if (id >= 0) { nrm[0] = B.normals[3 * (int64_t)id]; nrm[1] = B.normals[3 * (int64_t)id + 1]; nrm[2] = B.normals[3 * (int64_t)id + 2]; }
    return sdfk_icp::kept_plane(id, c.w, dmax, nrm);
}

// count and sum p of the kept points
__global__ __launch_bounds__(kBlock) void k_icpp_centre(IcpArgs A, IcpPlaneArgs B, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[4][kBlock];
    const float dmax = A.S->dist_max;
    double v[4];
    grid_sum(A.n, v, s, [&](int64_t i, double* acc) {
        float q[3], nrm[3];
        if (plane_cor(A, B, i, dmax, q, nrm)) {
            acc[0] += 1.0;
            acc[1] += A.points[3 * i]; acc[2] += A.points[3 * i + 1]; acc[3] += A.points[3 * i + 2];
        }
    });
    if (threadIdx.x == 0)
        for (int j = 0; j < 4; j++) B.P->part[blockIdx.x][j] = v[j];
}

__global__ __launch_bounds__(kBlock) void k_icpp_mean(IcpArgs A, IcpPlaneArgs B, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[4][kBlock];
    double r[4];
    sum_partials(B.P->part, 0, r, s);
    if (threadIdx.x != 0) return;
    for (int j = 0; j < 3; j++) A.S->pmean[j] = r[1 + j] / r[0];
    B.P->count = r[0];
}

// the normal equations: columns 0 .. 20 J_a J_b, 21 .. 26 J_a r, 27 r r
__global__ __launch_bounds__(kBlock) void k_icpp_nsum(IcpArgs A, IcpPlaneArgs B, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[kPlaneGroup][kBlock];
    const float dmax = A.S->dist_max;
    const double pm[3] = {A.S->pmean[0], A.S->pmean[1], A.S->pmean[2]};
    double v[kPlaneCols];
    grid_accumulate(A.n, v, [&](int64_t i, double* acc) {
        float q[3], nrm[3];
        if (!plane_cor(A, B, i, dmax, q, nrm)) return;
        const float p[3] = {A.points[3 * i], A.points[3 * i + 1], A.points[3 * i + 2]};
        double J[6], r;
        sdfk_icp::plane_row(p, q, nrm, pm, J, &r);
        int c = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) acc[c++] += J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; a++) acc[c++] += J[a] * r;
        acc[c] += r * r;
    });
#pragma unroll
    for (int c0 = 0; c0 < kPlaneCols; c0 += kPlaneGroup) {
        double grp[kPlaneGroup];
#pragma unroll
        for (int j = 0; j < kPlaneGroup; j++) grp[j] = v[c0 + j];
        block_sum(grp, s);
        if (threadIdx.x == 0)
            for (int j = 0; j < kPlaneGroup; j++) B.P->part[blockIdx.x][c0 + j] = grp[j];
        __syncthreads();   // (s is reused)
    }
}

// the solve (icp_solve.h) on one lane: the 6x6 Jacobi, the truncated solve, Cayley's rotation, convergence, the running total
__global__ __launch_bounds__(kBlock) void k_icpp_solve(IcpArgs A, IcpPlaneArgs B, int iter)
{
    if (icp_stopped(A.S, iter)) return;
    __shared__ double s[kPlaneGroup][kBlock];
    double red[kPlaneCols / kPlaneGroup][kPlaneGroup];
#pragma unroll
    for (int gq = 0; gq < kPlaneCols / kPlaneGroup; gq++) {
        sum_partials(B.P->part, gq * kPlaneGroup, red[gq], s);
        __syncthreads();   // (s is reused)
    }
    if (threadIdx.x != 0) return;
    double A21[21], b[6];
#pragma unroll
    for (int c = 0; c < 21; c++) A21[c] = red[c / kPlaneGroup][c % kPlaneGroup];
#pragma unroll
    for (int c = 0; c < 6; c++) b[c] = red[(21 + c) / kPlaneGroup][(21 + c) % kPlaneGroup];
    IcpState* S = A.S;
    float step[16], tot[16];
    bool conv;
    int retained;
    sdfk_icp::solve_step_plane(A21, b, S->pmean, S->total, A.conv_t, A.conv_r, step, tot, &conv, &retained);
    for (int q = 0; q < 16; q++) { S->step[q] = step[q]; S->total[q] = tot[q]; }
    B.P->rsq = red[27 / kPlaneGroup][27 % kPlaneGroup];
    B.P->retained = retained;
    S->iters = iter + 1;
    S->converged = conv;
    S->stop = conv || iter + 1 >= A.max_iters;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// the handle
// ---------------------------------------------------------------------------------------------------------------------------
// struct sdfk_points: points_set.h (shared with the other query files)

namespace {

void points_release(sdfk_points* s)
{
    dev_free(s->xyz);
    dev_free(s->sorted);
    dev_free(s->starts);
    s->xyz = nullptr;
    s->sorted = nullptr;
    s->starts = nullptr;
}

// Builds the search structure of s, whose sorted and starts are null, from s->xyz (synchronises: the host reads the bounding box
// to size the grid).  Refuses non-finite points.  s->sorted and s->starts are stored only when everything succeeded.
int points_build(sdfk_points* s, const char* who)
{
    const int64_t n = s->n;
    const unsigned bb = (unsigned)std::min<int64_t>(1024, (n + kBlock - 1) / kBlock);
    Staged st;
    float* part = st.scratch<float>((size_t)bb * 8);
    float* box_dev = st.scratch<float>(8);
    float box[8] = {};
    st.run([&] {
        ProfScope ps("k_pts_bounds");
        hipLaunchKernelGGL(k_pts_bounds, dim3(bb), dim3(kBlock), 0, g.stream, s->xyz, n, part);
        hipLaunchKernelGGL(k_pts_bounds_final, dim3(1), dim3(kBlock), 0, g.stream, part, (int)bb, box_dev);
    });
    st.run([&] { return hipMemcpyAsync(box, box_dev, 7 * sizeof(float), hipMemcpyDeviceToHost, g.stream); });
    st.run([&] { return hipMemcpyAsync(s->first, s->xyz, 3 * sizeof(float), hipMemcpyDeviceToHost, g.stream); });
    if (int r = st.finish(who)) return r;   // (synchronises: the box is read; its scratch goes back before the second phase)
    if (box[6] > 0) return fail(SDFK_ERR_INVALID, "%s: a static point has a NaN or infinite coordinate", who);

    s->G = grid_for_box(box, box + 3, n);
    s->cells = (int64_t)s->G.dim[0] * s->G.dim[1] * s->G.dim[2];
    const size_t cells = (size_t)s->cells;
    float4* sorted = st.kept<float4>((size_t)n);
    uint32_t* starts = st.kept<uint32_t>(cells + 1);
    uint32_t* keys = st.scratch<uint32_t>((size_t)n);
    uint32_t* cursor = st.scratch<uint32_t>(cells + 1);
    {
        ProfScope ps("k_pts_build");
        st.run([&] { return hipMemsetAsync(starts, 0, (cells + 1) * sizeof(uint32_t), g.stream); });
        st.run([&] { hipLaunchKernelGGL(k_pts_count, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, s->xyz, n, s->G, keys, starts); });
        st.run([&] { return sdfk_scan::scan(starts, s->cells, who); });
        st.run([&] { return hipMemcpyAsync(cursor, starts, cells * sizeof(uint32_t), hipMemcpyDeviceToDevice, g.stream); });
        st.run([&] { hipLaunchKernelGGL(k_pts_scatter, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, s->xyz, n, keys, cursor, sorted); });
    }
    if (int r = st.finish(who, false)) return r;   // (no wait: the queries that follow are queued behind the build)
    s->sorted = sorted;
    s->starts = starts;
    return SDFK_OK;
}

// Queues the search of nq device queries (caller order in and out).  `icp`/`iter`: the launch of an ICP iteration.
int points_search_launch(const sdfk_points* s, const float* q, int64_t nq, SearchOut O, const IcpState* icp, int iter)
{
    return sdfk_walk::walk_launch(s, nq, "k_pts_search", "points search", [&](unsigned long long* counter) {
        O.candidates = counter;
        hipLaunchKernelGGL(k_pts_search, dim3(grid_of(nq, kBlock)), dim3(kBlock), 0, g.stream, s->sorted, s->starts, s->G, s->first[0], s->first[1],
                           s->first[2], q, nq, O, icp, iter);
    }, /* counted = */ !icp);   // (not counted for ICP's launches)
}

int points_make(const void* pts, int64_t n, bool device, sdfk_points** out)
{
    if (int r = require_init()) return r;
    if (!out) return fail(SDFK_ERR_INVALID, "sdfk_points_create: null argument");
    *out = nullptr;
    if (n < 1) return fail(SDFK_ERR_INVALID, "sdfk_points_create: at least one point must be given");
    if (!pts) return fail(SDFK_ERR_INVALID, "sdfk_points_create: null points");
    if (n >= (int64_t(1) << 31)) return fail(SDFK_ERR_INVALID, "sdfk_points_create: 2^31 points or more");
    static const char* who = "sdfk_points_create";
    sdfk_points* s = new sdfk_points();
    s->n = n;
    Staged st;
    s->xyz = st.kept<float>((size_t)n * 3);
    st.run([&] { return hipMemcpyAsync(s->xyz, pts, (size_t)n * 3 * sizeof(float), device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, g.stream); });
    st.run([&] { return points_build(s, who); });   // (synchronises: the caller's host array is not retained)
    if (int r = st.finish(who, false)) {
        delete s;   // (nothing to release: finish() freed xyz, and a build that failed stored nothing)
        return r;
    }
    *out = s;
    return SDFK_OK;
}

int points_append(sdfk_points* s, const void* pts, int64_t n, bool device)
{
    if (int r = require_init()) return r;
    if (!s || n < 0 || (n > 0 && !pts)) return fail(SDFK_ERR_INVALID, "sdfk_points_add: null / negative argument");
    if (s->n + n >= (int64_t(1) << 31)) return fail(SDFK_ERR_INVALID, "sdfk_points_add: 2^31 static points or more");
    if (n == 0) return SDFK_OK;
    // the concatenation, rebuilt; on a refusal the set stays as it was
    static const char* who = "sdfk_points_add";
    sdfk_points t = *s;
    t.n = s->n + n;
    t.sorted = nullptr;
    t.starts = nullptr;
    Staged st;
    t.xyz = st.kept<float>((size_t)t.n * 3);
    st.run([&] { return hipMemcpyAsync(t.xyz, s->xyz, (size_t)s->n * 3 * sizeof(float), hipMemcpyDeviceToDevice, g.stream); });
    st.run([&] {
        return hipMemcpyAsync(t.xyz + s->n * 3, pts, (size_t)n * 3 * sizeof(float), device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, g.stream);
    });
    st.run([&] { return points_build(&t, who); });
    if (int r = st.finish(who, false)) return r;   // (nothing of t to release: finish() freed its xyz, and a build that failed stored nothing)
    points_release(s);
    *s = t;
    return SDFK_OK;
}

// `normals_dev` null: point to point.  Otherwise point to plane with one normal per static point; `stats` (may be null) receives its int64[4].
int icp_run(sdfk_points* s, const sdfk_icp_params* prm, const float* normals_dev, float* pts_dev, int64_t n, float total[16], int32_t* iterations,
            int64_t* stats = nullptr)
{
    const bool plane = normals_dev != nullptr;
    Staged st;
    IcpState* S = st.scratch<IcpState>(1);
    float4* cor = st.scratch<float4>((size_t)n);
    IcpPlane* P = plane ? st.scratch<IcpPlane>(1) : nullptr;
    int32_t* index = plane ? st.scratch<int32_t>((size_t)n) : nullptr;
    IcpPlaneArgs B{index, normals_dev, P};
    struct { double count, rsq; int retained; } host_plane{};
    IcpArgs A{pts_dev, cor, n, prm->good_correspondence_distance, prm->converged_max_translation, prm->converged_max_rotation, prm->max_iterations, S};
    struct { float total[16]; int iters, stop, converged; } host{};
    for (int q = 0; q < 16; q++) host.total[q] = (q % 5 == 0) ? 1.0f : 0.0f;
    if (prm->max_iterations > 0) {
        st.run([&] { hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, g.stream, S); });
        // Iterations are queued in chunks; the launches of an iteration after the one that stopped the registration exit at once
        // (they read the device flag), and the host looks at the flag between chunks.
        constexpr int kChunk = 4;
        for (int it0 = 0; st.ok() && it0 < prm->max_iterations; it0 += kChunk) {
            for (int it = it0; st.ok() && it < std::min(it0 + kChunk, prm->max_iterations); it++) {
                st.run([&] { return points_search_launch(s, pts_dev, n, SearchOut{index, nullptr, nullptr, cor, nullptr}, S, it); });
                st.run([&] {
                    ProfScope ps(plane ? "k_icpp_step" : "k_icp_step");
                    launch_grid_sum(k_icp_dsum, g.stream, A, it);
                    launch_grid_sum(k_icp_dvar, g.stream, A, it);
                    hipLaunchKernelGGL(k_icp_dstats, dim3(1), dim3(kBlock), 0, g.stream, A, it);
                    if (plane) {
                        launch_grid_sum(k_icpp_centre, g.stream, A, B, it);
                        hipLaunchKernelGGL(k_icpp_mean, dim3(1), dim3(kBlock), 0, g.stream, A, B, it);
                        launch_grid_sum(k_icpp_nsum, g.stream, A, B, it);
                        hipLaunchKernelGGL(k_icpp_solve, dim3(1), dim3(kBlock), 0, g.stream, A, B, it);
                    } else {
                        launch_grid_sum(k_icp_fsum, g.stream, A, it);
                        hipLaunchKernelGGL(k_icp_means, dim3(1), dim3(kBlock), 0, g.stream, A, it);
                        launch_grid_sum(k_icp_csum, g.stream, A, it);
                        hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(kBlock), 0, g.stream, A, it);
                    }
                    hipLaunchKernelGGL(k_icp_apply, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, g.stream, A, it);
                });
            }
            if (plane) st.run([&] { return hipMemcpyAsync(&host_plane, &P->count, sizeof host_plane, hipMemcpyDeviceToHost, g.stream); });
            st.read(&host, &S->total, sizeof host);
            if (host.stop) break;
        }
    }
    if (int r = st.finish("sdfk_icp_register", false)) return r;
    for (int q = 0; q < 16; q++) total[q] = host.total[q];
    *iterations = host.iters;
    if (stats) {   // (of the last iteration run; no iteration: zeros)
        stats[0] = (int64_t)host_plane.count;
        stats[1] = (int64_t)sdfk_icp::f64_bits(host_plane.rsq);
        stats[2] = host.converged;
        stats[3] = host_plane.retained;
    }
    return SDFK_OK;
}

int icp_check(sdfk_points* s, const sdfk_icp_params* prm, const void* pts, int64_t n, float* total, int32_t* iterations)
{
    if (int r = require_init()) return r;
    if (!s || !prm || !total || !iterations || n < 0 || (n > 0 && !pts)) return fail(SDFK_ERR_INVALID, "sdfk_icp_register: null / negative argument");
    if (n == 0) return fail(SDFK_ERR_INVALID, "sdfk_icp_register: no dynamic points");
    if (n >= (int64_t(1) << 31)) return fail(SDFK_ERR_INVALID, "sdfk_icp_register: 2^31 points or more");
    if (prm->max_iterations < 0) return fail(SDFK_ERR_INVALID, "sdfk_icp_register: negative max_iterations");
    return SDFK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int sdfk_points_create(const float* points3, int64_t n, sdfk_points** out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return points_make(points3, n, false, out);
}

extern "C" int sdfk_points_create_device(const void* points3_dev, int64_t n, sdfk_points** out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return points_make(points3_dev, n, true, out);
}

extern "C" int sdfk_points_add(sdfk_points* s, const float* points3, int64_t n)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return points_append(s, points3, n, false);
}

extern "C" int sdfk_points_add_device(sdfk_points* s, const void* points3_dev, int64_t n)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return points_append(s, points3_dev, n, true);
}

extern "C" int sdfk_points_count(const sdfk_points* s, int64_t* n)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);   // (sdfk_points_add replaces the set under the lock)
    if (!s || !n) return fail(SDFK_ERR_INVALID, "sdfk_points_count: null argument");
    *n = s->n;
    return SDFK_OK;
}

extern "C" int sdfk_points_stats(const sdfk_points* s, int64_t stats[5])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!s || !stats) return fail(SDFK_ERR_INVALID, "sdfk_points_stats: null argument");
    stats[0] = s->G.dim[0];
    stats[1] = s->G.dim[1];
    stats[2] = s->G.dim[2];
    stats[3] = s->last_candidates;
    stats[4] = s->last_queries;
    return SDFK_OK;
}

extern "C" int sdfk_points_search_device(const sdfk_points* s, const void* queries3_dev, int64_t n, void* index_dev, void* distance_dev,
                                         void* nearest3_dev)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = require_init()) return r;
    if (!s || n < 0 || (n > 0 && !queries3_dev)) return fail(SDFK_ERR_INVALID, "sdfk_points_search: null / negative argument");
    if (n >= (int64_t(1) << 32)) return fail(SDFK_ERR_INVALID, "sdfk_points_search: 2^32 queries or more");
    if (n == 0) return SDFK_OK;
    SearchOut O{(int32_t*)index_dev, (float*)distance_dev, (float*)nearest3_dev, nullptr, nullptr};
    return points_search_launch(s, (const float*)queries3_dev, n, O, nullptr, 0);
}

extern "C" int sdfk_points_search(const sdfk_points* s, const float* queries3, int64_t n, int32_t* index, float* distance, float* nearest3)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = require_init()) return r;
    if (!s || n < 0 || (n > 0 && !queries3)) return fail(SDFK_ERR_INVALID, "sdfk_points_search: null / negative argument");
    if (n >= (int64_t(1) << 32)) return fail(SDFK_ERR_INVALID, "sdfk_points_search: 2^32 queries or more");
    if (n == 0) return SDFK_OK;
    Staged st;
    const float* qd = st.in(queries3, (size_t)n * 3);
    const SearchOut O{st.out(index, (size_t)n), st.out(distance, (size_t)n), st.out(nearest3, (size_t)n * 3), nullptr, nullptr};
    st.run([&] { return points_search_launch(s, qd, n, O, nullptr, 0); });
    return st.finish("sdfk_points_search");
}

extern "C" int sdfk_icp_register_device(sdfk_points* s, const sdfk_icp_params* prm, void* points3_dev, int64_t n, float total[16],
                                        int32_t* iterations)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = icp_check(s, prm, points3_dev, n, total, iterations)) return r;
    return icp_run(s, prm, nullptr, (float*)points3_dev, n, total, iterations);
}

extern "C" int sdfk_icp_register(sdfk_points* s, const sdfk_icp_params* prm, float* points3, int64_t n, float total[16], int32_t* iterations)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = icp_check(s, prm, points3, n, total, iterations)) return r;
    for (int64_t i = 0; i < 3 * n; i++)   // (as static sets are: nothing is touched)
        if (!std::isfinite(points3[i])) return fail(SDFK_ERR_INVALID, "sdfk_icp_register: dynamic point %lld has a NaN or infinite coordinate", (long long)(i / 3));
    Staged st;
    float* pd = st.inout(points3, (size_t)n * 3);
    st.run([&] { return icp_run(s, prm, nullptr, pd, n, total, iterations); });
    return st.finish("sdfk_icp_register");
}

extern "C" int sdfk_icp_register_plane_device(sdfk_points* s, const sdfk_icp_params* prm, const void* normals3_dev, void* points3_dev, int64_t n,
                                              float total[16], int32_t* iterations, int64_t stats[4])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = icp_check(s, prm, points3_dev, n, total, iterations)) return r;
    if (!normals3_dev) return fail(SDFK_ERR_INVALID, "sdfk_icp_register_plane: null normals");
    return icp_run(s, prm, (const float*)normals3_dev, (float*)points3_dev, n, total, iterations, stats);
}

extern "C" int sdfk_icp_register_plane(sdfk_points* s, const sdfk_icp_params* prm, const float* normals3, float* points3, int64_t n, float total[16],
                                       int32_t* iterations, int64_t stats[4])
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = icp_check(s, prm, points3, n, total, iterations)) return r;
    if (!normals3) return fail(SDFK_ERR_INVALID, "sdfk_icp_register_plane: null normals");
    for (int64_t i = 0; i < 3 * n; i++)   // (nothing is touched)
        if (!std::isfinite(points3[i])) return fail(SDFK_ERR_INVALID, "sdfk_icp_register_plane: dynamic point %lld has a NaN or infinite coordinate", (long long)(i / 3));
    for (int64_t i = 0; i < 3 * s->n; i++)
        if (!std::isfinite(normals3[i])) return fail(SDFK_ERR_INVALID, "sdfk_icp_register_plane: normal %lld has a NaN or infinite component", (long long)(i / 3));
    Staged st;
    float* pd = st.inout(points3, (size_t)n * 3);
    const float* nd = st.in(normals3, (size_t)s->n * 3);
    float tot[16];   // (the caller's results are written once everything, the copy back included, succeeded)
    int32_t iters = 0;
    int64_t stt[4] = {0, 0, 0, 0};
    st.run([&] { return icp_run(s, prm, nd, pd, n, tot, &iters, stt); });
    if (int r = st.finish("sdfk_icp_register_plane")) return r;
    for (int q = 0; q < 16; q++) total[q] = tot[q];
    *iterations = iters;
    if (stats)
        for (int q = 0; q < 4; q++) stats[q] = stt[q];
    return SDFK_OK;
}

extern "C" void sdfk_points_free(sdfk_points* s)
{
    StateScope in_owner_context(s ? s->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    bind_thread();
    if (!s) return;
    if (g.inited) points_release(s);
    delete s;
}
