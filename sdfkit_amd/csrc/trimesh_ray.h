// trimesh_ray.h -- the arithmetic of sdfk_trimesh_raycast / sdfk_trimesh_render (lib_trimesh_ray.hip): the per-ray set-up, the
// watertight ray-triangle test of Woop, Benthin and Wald (2013) in binary64, the (t, index) order of hits, the clip of a ray against
// the grid's box, the walk of the handle's uniform grid along a ray, the camera ray of a pixel and the shading of a hit.  Plain C++
// outside hipcc (no contraction: -ffp-contract=off), so that a host program runs the very walk the kernels run
// (tests/cpp/mesh_ray_host.cpp) and is compared with brute force over all triangles.
//
// THE WALK, and why it finds what brute force finds.  Write S for the walk's slack: twice (Grid::slack + max|o| 2^-45).  Grid::slack
// bounds the error of cell assignment: cell_of(x) == s implies F(s) - slack <= x <= F(s + 1) + slack for the nominal faces
// F(s) = lo + (float)s * h, and cell_of is monotone.  The second term bounds, with a factor 2^7 to spare, the rounding of the
// binary64 positions o + t d and of the slab parameters below, which are relative 2^-52 of |o| + |t d|; the factor two leaves
// room for the f32 rounding of a widened position ((|lo| + |hi|) 2^-24 < slack / 16) and for the binary64 error of the hit itself.
// A triangle that the test reports hit at parameter t has the point p = o + t d within that error of itself, hence of its own
// f32 box [lo3, hi3], and is binned in every cell of cell_of(lo3) .. cell_of(hi3) per axis.
//  1. Clip: p lies in the box of all triangles, so t lies in the ray's interval [t0, t1] inside the box widened by S (an axis
//     with d == 0 only decides whether the ray misses the box).  A ray that misses the widened box hits nothing.
//  2. Slabs along the dominant axis kz (greatest |d|, so the other coordinates move less than kz's does).  Slab s gets the
//     parameter interval I(s) in which kz's coordinate is within [F(s) - S, F(s + 1) + S], unbounded below for the first cell of
//     the axis and above for the last (cell_of clamps), cut to [t0, t1].  The nominal cells tile the axis and the triangle's cells
//     c0 .. c1 cover its extent up to slack, so SOME s in c0 .. c1 has t in I(s).
//  3. In slab s the walk takes the ray's box over I(s), widens it by S, and visits every cell of cell_of(low) .. cell_of(high) in
//     the two other axes: by monotonicity that range meets the triangle's on each axis, since p's coordinate is inside both
//     intervals.  So in the slab of step 2 the walk visits a cell that lists the triangle.  Each x run of the rectangle is one
//     contiguous range of `list` (starts is x-fastest).
//  4. The pre-test rejects a triangle whose f32 box misses the slab's widened ray box.  In the slab of step 2 the boxes share p,
//     so the triangle is tested there, in binary64, with the one test every other visit would run: the answer does not depend
//     on the cell it was found from, and a triangle tested more than once changes nothing under the (t, index) minimum.
//  5. Early exit: after slab s every untested hit lies in some later I(s'), whose lower end is at least the next slab's; the walk
//     stops only when the best t is strictly below that end, so no later hit can win or tie.  A hit is accepted whatever slab it
//     was found from (triangles span cells); "stop at the first cell with a hit" would be wrong.
// What the argument does not cover: a ray lying in a triangle's plane to within binary64 rounding can pass the sign test on noise
// and get a quotient t unrelated to the geometry.  Brute force reports such a hit wherever t falls; the walk reports it when t
// falls where the ray is near the triangle, or when any visited cell lists the triangle.  An exactly coplanar ray has det == 0.
#pragma once
#include "points_grid.h"

#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SDFK_RAY_HD __host__ __device__ __forceinline__
#else
#define SDFK_RAY_HD inline
#endif

namespace sdfk_trimesh_ray {

using sdfk_points_grid::Grid;
using sdfk_points_grid::cell_of;

// (ternaries, not indexing by a per-lane value: the arrays stay in registers)
SDFK_RAY_HD double pick(const double v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }
SDFK_RAY_HD float pickf(const float v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }
SDFK_RAY_HD int picki(const int v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }
SDFK_RAY_HD bool finite32(float x) { return __builtin_fabsf(x) <= FLT_MAX; }   // (false for NaN)

struct Ray {
    double o[3], d[3];
    double Sx, Sy, Sz;
    double tmin, tmax;
    int kx, ky, kz;
    bool ok;   // every component finite and some direction component non-zero; otherwise the ray is a miss
};

struct Hit {
    double t, U, V, W, det;
    int tri;   // -1: none
};

SDFK_RAY_HD Hit no_hit()
{
    Hit H;
    H.t = (double)INFINITY;
    H.U = H.V = H.W = H.det = 0.0;
    H.tri = -1;
    return H;
}

SDFK_RAY_HD Ray ray_setup(const float o[3], const float d[3], double tmin, double tmax)
{
    Ray R;
    R.ok = true;
    for (int a = 0; a < 3; a++) {
        R.o[a] = (double)o[a];
        R.d[a] = (double)d[a];
        if (!finite32(o[a]) || !finite32(d[a])) R.ok = false;
    }
    if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) R.ok = false;
    R.tmin = tmin;
    R.tmax = tmax;
    const double ax = __builtin_fabs(R.d[0]), ay = __builtin_fabs(R.d[1]), az = __builtin_fabs(R.d[2]);
    int kz = 0;   // the axis of greatest |d|, ties to the lowest
    double am = ax;
    if (ay > am) { kz = 1; am = ay; }
    if (az > am) { kz = 2; am = az; }
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const double dz = pick(R.d, kz);
    if (dz < 0.0) { const int s = kx; kx = ky; ky = s; }
    R.kx = kx; R.ky = ky; R.kz = kz;
    R.Sx = pick(R.d, kx) / dz;
    R.Sy = pick(R.d, ky) / dz;
    R.Sz = 1.0 / dz;
    return R;
}

// The watertight test: true for a hit in [tmin, tmax], with its t and U, V, W, det.
SDFK_RAY_HD bool ray_triangle(const Ray& R, const float a[3], const float b[3], const float c[3], double* t, double uvwd[4])
{
    const double A[3] = {(double)a[0] - R.o[0], (double)a[1] - R.o[1], (double)a[2] - R.o[2]};
    const double B[3] = {(double)b[0] - R.o[0], (double)b[1] - R.o[1], (double)b[2] - R.o[2]};
    const double C[3] = {(double)c[0] - R.o[0], (double)c[1] - R.o[1], (double)c[2] - R.o[2]};
    const double Az = pick(A, R.kz), Bz = pick(B, R.kz), Cz = pick(C, R.kz);
    const double Ax = pick(A, R.kx) - R.Sx * Az, Ay = pick(A, R.ky) - R.Sy * Az;
    const double Bx = pick(B, R.kx) - R.Sx * Bz, By = pick(B, R.ky) - R.Sy * Bz;
    const double Cx = pick(C, R.kx) - R.Sx * Cz, Cy = pick(C, R.ky) - R.Sy * Cz;
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;
    const double det = (U + V) + W;
    if (det == 0.0) return false;
    const double T = (U * (R.Sz * Az) + V * (R.Sz * Bz)) + W * (R.Sz * Cz);
    const double tt = T / det;
    if (!(tt >= R.tmin && tt <= R.tmax && __builtin_fabs(tt) <= DBL_MAX)) return false;   // (a NaN is a miss)
    *t = tt;
    uvwd[0] = U; uvwd[1] = V; uvwd[2] = W; uvwd[3] = det;
    return true;
}

SDFK_RAY_HD bool hit_before(double t, int tri, const Hit& H) { return t < H.t || (t == H.t && tri < H.tri); }

// What the walk hands its ranges of `list` to: the pre-test, the binary64 test, the minimum.  Tris gives box(t, lo3, hi3) and
// corners(t, a, b, c).  ANY: stop at the first hit.
template <class Tris, bool ANY>
struct Caster {
    const Tris& T;
    const uint32_t* list;
    const Ray& R;
    Hit best;
    unsigned long long tests;

    SDFK_RAY_HD Caster(const Tris& tris, const uint32_t* l, const Ray& r) : T(tris), list(l), R(r), best(no_hit()), tests(0) {}

    SDFK_RAY_HD double bound() const { return best.t; }

    // true: the walk may end
    SDFK_RAY_HD bool range(uint32_t j0, uint32_t j1, const double seglo[3], const double seghi[3])
    {
        for (uint32_t j = j0; j < j1; j++) {
            const uint32_t t = list[j];
            float lo[3], hi[3];
            T.box(t, lo, hi);
            if ((double)lo[0] > seghi[0] || (double)hi[0] < seglo[0] || (double)lo[1] > seghi[1] || (double)hi[1] < seglo[1] ||
                (double)lo[2] > seghi[2] || (double)hi[2] < seglo[2])
                continue;
            float a[3], b[3], c[3];
            T.corners(t, a, b, c);
            double tt, q[4];
            tests++;
            if (!ray_triangle(R, a, b, c, &tt, q)) continue;
            if (ANY) {
                best.t = tt;
                best.tri = 0;
                return true;
            }
            if (hit_before(tt, (int)t, best)) {   // (the first hit too: no_hit() has t = +inf)
                best.t = tt; best.U = q[0]; best.V = q[1]; best.W = q[2]; best.det = q[3];
                best.tri = (int)t;
            }
        }
        return false;
    }
};

SDFK_RAY_HD double walk_slack(const Grid& G, const Ray& R)
{
    const double om = fmax(__builtin_fabs(R.o[0]), fmax(__builtin_fabs(R.o[1]), __builtin_fabs(R.o[2])));
    return 2.0 * ((double)G.slack + om * 0x1p-45);
}

// The ray's interval inside the box of the grid widened by S, cut to [tmin, tmax]; false: the ray misses it.
SDFK_RAY_HD bool clip_to_box(const Grid& G, const Ray& R, double S, double* t0, double* t1)
{
    double u0 = R.tmin, u1 = R.tmax;
    for (int a = 0; a < 3; a++) {
        const double lo = (double)G.lo[a] - S, hi = (double)G.hi[a] + S;
        if (R.d[a] == 0.0) {
            if (!(R.o[a] >= lo && R.o[a] <= hi)) return false;
        } else {
            const double inv = 1.0 / R.d[a];
            const double ta = (lo - R.o[a]) * inv, tb = (hi - R.o[a]) * inv;
            u0 = fmax(u0, fmin(ta, tb));
            u1 = fmin(u1, fmax(ta, tb));
        }
    }
    *t0 = u0;
    *t1 = u1;
    return u0 <= u1;
}

// The walk (see the head of this file).  V: bool range(j0, j1, seglo, seghi), double bound().
template <class V>
SDFK_RAY_HD void walk(const Grid& G, const uint32_t* starts, const Ray& R, V& vis)
{
    if (!R.ok) return;
    const double S = walk_slack(G, R);
    double t0, t1;
    if (!clip_to_box(G, R, S, &t0, &t1)) return;
    const int kz = R.kz;
    const double oz = pick(R.o, kz), dz = pick(R.d, kz), iz = R.Sz;
    const float glo = pickf(G.lo, kz);
    const int gdim = picki(G.dim, kz);
    const bool up = dz > 0.0;
    const double zA = oz + t0 * dz, zB = oz + t1 * dz;
    int s = cell_of((float)(up ? zA - S : zA + S), glo, G.inv_h, gdim);
    const int s_end = cell_of((float)(up ? zB + S : zB - S), glo, G.inv_h, gdim);
    const uint32_t gx = (uint32_t)G.dim[0], gy = (uint32_t)G.dim[1];
    for (;;) {
        const float f0 = glo + (float)s * G.h, f1 = glo + (float)(s + 1) * G.h;
        const double fnear = up ? (double)f0 - S : (double)f1 + S, ffar = up ? (double)f1 + S : (double)f0 - S;
        const bool first = up ? s == 0 : s == gdim - 1, last = up ? s == gdim - 1 : s == 0;
        const double ta = first ? t0 : fmax(t0, (fnear - oz) * iz);
        const double tb = last ? t1 : fmin(t1, (ffar - oz) * iz);
        if (ta <= tb) {
            double seglo[3], seghi[3];
            int c0[3], c1[3];
            for (int a = 0; a < 3; a++) {
                const double pa = R.o[a] + ta * R.d[a], pb = R.o[a] + tb * R.d[a];
                seglo[a] = fmin(pa, pb) - S;
                seghi[a] = fmax(pa, pb) + S;
                c0[a] = cell_of((float)seglo[a], G.lo[a], G.inv_h, G.dim[a]);
                c1[a] = cell_of((float)seghi[a], G.lo[a], G.inv_h, G.dim[a]);
                if (a == kz) c0[a] = c1[a] = s;
            }
            for (int z = c0[2]; z <= c1[2]; z++)
                for (int y = c0[1]; y <= c1[1]; y++) {
                    const uint32_t row = ((uint32_t)z * gy + (uint32_t)y) * gx;
                    if (vis.range(starts[row + (uint32_t)c0[0]], starts[row + (uint32_t)c1[0] + 1u], seglo, seghi)) return;
                }
        }
        if (s == s_end) return;
        // every untested hit has t >= the next slab's entry
        const double tnext = up ? ((double)f1 - S - oz) * iz : ((double)f0 + S - oz) * iz;
        if (vis.bound() < tnext) return;
        s += up ? 1 : -1;
    }
}

// ---- the camera ray of pixel (i, j): the arithmetic of the sdfk_raymarch kernel (sample_codegen.h, "GetCameraRays"), copied op
// for op in f32: x, y, the matrix product, the divide by w, the subtraction of the camera, v / length.
SDFK_RAY_HD void camera_ray(const float cam[3], const float m[16], int width, int height, int i, int j, float r[3])
{
    const float y = 1.0f - 2.0f * (float)j / (float)(height - 1);
    const float x = -1.0f + 2.0f * (float)i / (float)(width - 1);
    float v4[4];
    for (int q = 0; q < 4; q++) v4[q] = ((x * m[q] + y * m[4 + q]) + 0.0f * m[8 + q]) + 1.0f * m[12 + q];
    const float dx = v4[0] / v4[3] - cam[0], dy = v4[1] / v4[3] - cam[1], dz = v4[2] / v4[3] - cam[2];
    const float dl = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
    r[0] = dx / dl; r[1] = dy / dl; r[2] = dz / dl;
}

// the f32 outputs of a hit
SDFK_RAY_HD void hit_outputs(const Hit& H, float* distance, float w[3])
{
    *distance = (float)H.t;
    w[0] = (float)(H.U / H.det);
    w[1] = (float)(H.V / H.det);
    w[2] = (float)(H.W / H.det);
}

SDFK_RAY_HD void normalize_inplace(float& x, float& y, float& z)   // sdfk_normalize_inplace of sample_codegen.h
{
    const float len = __builtin_sqrtf((x * x + y * y) + z * z);
    if (len > 0.0f) {
        const float r = 1.0f / len;
        x = x * r; y = y * r; z = z * r;
    }
}

// Lambert shading of a hit with the ray marcher's constants: cam, the unit ray r, the f32 distance and weights, the triangle's
// corners and the colours of its vertices (null: white).
SDFK_RAY_HD void shade(const float cam[3], const float r[3], float distance, const float w[3], const float a[3], const float b[3],
                       const float c[3], const float* ca, const float* cb, const float* cc, float rgb[3])
{
    const float sx = cam[0] + r[0] * distance, sy = cam[1] + r[1] * distance, sz = cam[2] + r[2] * distance;
    const double e1[3] = {(double)b[0] - (double)a[0], (double)b[1] - (double)a[1], (double)b[2] - (double)a[2]};
    const double e2[3] = {(double)c[0] - (double)a[0], (double)c[1] - (double)a[1], (double)c[2] - (double)a[2]};
    const double n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2], n2 = e1[0] * e2[1] - e1[1] * e2[0];
    const double len = __builtin_sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (len > 0.0) { nx = (float)(n0 / len); ny = (float)(n1 / len); nz = (float)(n2 / len); }
    if ((nx * r[0] + ny * r[1]) + nz * r[2] > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    float lx = 5.0f - sx, ly = 5.0f - sy, lz = 10.0f - sz;
    normalize_inplace(lx, ly, lz);
    const float nl = (nx * lx + ny * ly) + nz * lz;
    const float dv = nl != nl ? nl : (nl > 0.0f ? nl : 0.0f);   // the IEEE maximum of (n.l, 0)
    for (int k = 0; k < 3; k++) {
        const float col = ca ? (ca[k] * w[0] + cb[k] * w[1]) + cc[k] * w[2] : 1.0f;
        rgb[k] = dv * col + 0.1f;
    }
}

}  // namespace sdfk_trimesh_ray
