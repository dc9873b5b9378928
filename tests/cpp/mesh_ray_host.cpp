// mesh_ray_host.cpp -- runs sdfkit_amd/csrc/trimesh_ray.h (the set-up, the test, the clip and THE WALK the kernels of
// lib_trimesh_ray.hip run, the camera ray and the shading) on the host, over a grid rebuilt as lib_trimesh.hip builds it
// (points_grid.h grid_for_box / cell_of, every cell a triangle's f32 box overlaps), for tests/test_mesh_ray_host.py to compare
// with the numpy model.  The program also runs the header's own brute force and counts the rays on which the walk differs from it.
// usage: mesh_ray_host MODE in out
//   cast    in: int64 nv, nt, n, flags; f32 tmin, tmax; f32 V[3 nv]; int32 T[3 nt]; f32 O[3 n]; f32 D[3 n]
//           out (int64): 0, binary64 tests of the walk, rays where walk != brute force, dim x, y, z, triangle-cell pairs, n;
//                        then per ray: triangle, the bits of distance, of the three weights, the ray's own test count
//   render  in: int64 nv, nt, width, height, has_colors; f32 near, far, cam[3], m[16]; f32 V[3 nv]; int32 T[3 nt]; f32 colours[3 nv]
//           out (int64): the same eight; then per pixel: triangle, the bits of depth, of r, g, b, the pixel's test count
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sdfkit_amd/csrc/trimesh_ray.h"

using namespace sdfk_trimesh_ray;

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

static int64_t bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    return (int64_t)u;
}

struct HostTris {
    std::vector<float> p, lo, hi;   // 9, 3, 3 per triangle
    void box(uint32_t t, float l[3], float h[3]) const
    {
        for (int a = 0; a < 3; a++) { l[a] = lo[3 * (size_t)t + a]; h[a] = hi[3 * (size_t)t + a]; }
    }
    void corners(uint32_t t, float a[3], float b[3], float c[3]) const
    {
        const float* q = &p[9 * (size_t)t];
        for (int k = 0; k < 3; k++) { a[k] = q[k]; b[k] = q[3 + k]; c[k] = q[6 + k]; }
    }
};

struct HostMesh {
    HostTris tris;
    Grid G;
    std::vector<uint32_t> starts, list;
    int64_t nt = 0;
};

// what k_tm_pack, k_tm_bounds, grid_for_box and the binning kernels make (the order inside a cell is the triangle order here; on
// the device it is whatever the atomics gave, which no first-hit answer or count depends on)
static void build(HostMesh& M, const float* V, const int32_t* T, int64_t nt)
{
    M.nt = nt;
    M.tris.p.resize(9 * (size_t)nt);
    M.tris.lo.resize(3 * (size_t)nt);
    M.tris.hi.resize(3 * (size_t)nt);
    float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t t = 0; t < nt; t++)
        for (int a = 0; a < 3; a++) {
            float c[3];
            for (int k = 0; k < 3; k++) c[k] = M.tris.p[9 * t + 3 * k + a] = V[3 * (int64_t)T[3 * t + k] + a];
            const float lo = fminf(fminf(c[0], c[1]), c[2]), hi = fmaxf(fmaxf(c[0], c[1]), c[2]);
            M.tris.lo[3 * t + a] = lo;
            M.tris.hi[3 * t + a] = hi;
            blo[a] = fminf(blo[a], lo);
            bhi[a] = fmaxf(bhi[a], hi);
        }
    M.G = sdfk_points_grid::grid_for_box(blo, bhi, nt);
    const Grid& G = M.G;
    const size_t cells = (size_t)G.dim[0] * G.dim[1] * G.dim[2];
    M.starts.assign(cells + 1, 0);
    auto each = [&](auto&& f) {
        for (int64_t t = 0; t < nt; t++) {
            int c0[3], c1[3];
            for (int a = 0; a < 3; a++) {
                c0[a] = cell_of(M.tris.lo[3 * t + a], G.lo[a], G.inv_h, G.dim[a]);
                c1[a] = cell_of(M.tris.hi[3 * t + a], G.lo[a], G.inv_h, G.dim[a]);
            }
            for (int z = c0[2]; z <= c1[2]; z++)
                for (int y = c0[1]; y <= c1[1]; y++)
                    for (int x = c0[0]; x <= c1[0]; x++) f(((size_t)z * G.dim[1] + y) * G.dim[0] + x, (uint32_t)t);
        }
    };
    each([&](size_t c, uint32_t) { M.starts[c + 1]++; });
    for (size_t c = 0; c < cells; c++) M.starts[c + 1] += M.starts[c];
    M.list.resize(M.starts[cells]);
    std::vector<uint32_t> cursor(M.starts.begin(), M.starts.end() - 1);
    each([&](size_t c, uint32_t t) { M.list[cursor[c]++] = t; });
}

// Brute force over triangles 0 .. nt - 1 with the header's test and order: this program's own reference next to the numpy model.
template <class Tris, bool ANY>
static Hit brute(const Tris& T, int64_t nt, const Ray& R)
{
    Hit best = no_hit();
    if (!R.ok) return best;
    for (int64_t t = 0; t < nt; t++) {
        float a[3], b[3], c[3];
        T.corners((uint32_t)t, a, b, c);
        double tt, q[4];
        if (!ray_triangle(R, a, b, c, &tt, q)) continue;
        if (ANY) { best.t = tt; best.tri = 0; return best; }
        if (hit_before(tt, (int)t, best)) {   // (the first hit too: no_hit() has t = +inf)
            best.t = tt; best.U = q[0]; best.V = q[1]; best.W = q[2]; best.det = q[3];
            best.tri = (int)t;
        }
    }
    return best;
}

static bool same(const Hit& a, const Hit& b, bool any)
{
    if (a.tri != b.tri) return false;
    if (any || a.tri < 0) return true;
    return a.t == b.t && a.U == b.U && a.V == b.V && a.W == b.W && a.det == b.det;
}

template <bool ANY>
static Hit cast_one(const HostMesh& M, const Ray& R, unsigned long long* tests, int64_t* differs)
{
    Caster<HostTris, ANY> C(M.tris, M.list.data(), R);
    walk(M.G, M.starts.data(), R, C);
    *tests = C.tests;
    const Hit B = brute<HostTris, ANY>(M.tris, M.nt, R);
    if (!same(C.best, B, ANY)) ++*differs;
    return C.best;
}

static void head(std::vector<int64_t>& out, const HostMesh& M, int64_t n)
{
    out.assign(8, 0);
    out[3] = M.G.dim[0]; out[4] = M.G.dim[1]; out[5] = M.G.dim[2];
    out[6] = (int64_t)M.list.size();
    out[7] = n;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const std::string mode = argv[1];
    const std::vector<char> in = slurp(argv[2]);
    std::vector<int64_t> out;
    HostMesh M;
    if (mode == "cast") {
        int64_t h[4];
        float r[2];
        if (in.size() < sizeof h + sizeof r) return 3;
        memcpy(h, in.data(), sizeof h);
        memcpy(r, in.data() + sizeof h, sizeof r);
        const int64_t nv = h[0], nt = h[1], n = h[2], flags = h[3];
        if (in.size() != sizeof h + sizeof r + 4 * (size_t)(3 * nv + 3 * nt + 6 * n)) return 3;
        const float* V = (const float*)(in.data() + sizeof h + sizeof r);
        const int32_t* T = (const int32_t*)(V + 3 * nv);
        const float* O = (const float*)(T + 3 * nt);
        const float* D = O + 3 * n;
        build(M, V, T, nt);
        head(out, M, n);
        for (int64_t i = 0; i < n; i++) {
            const Ray R = ray_setup(O + 3 * i, D + 3 * i, (double)r[0], (double)r[1]);
            unsigned long long tests = 0;
            const Hit H = (flags & 1) ? cast_one<true>(M, R, &tests, &out[2]) : cast_one<false>(M, R, &tests, &out[2]);
            float dist = INFINITY, w[3] = {NAN, NAN, NAN};
            if (!(flags & 1) && H.tri >= 0) hit_outputs(H, &dist, w);
            out[1] += (int64_t)tests;
            out.insert(out.end(), {(int64_t)H.tri, bits(dist), bits(w[0]), bits(w[1]), bits(w[2]), (int64_t)tests});
        }
    } else if (mode == "render") {
        int64_t h[5];
        float r[21];
        if (in.size() < sizeof h + sizeof r) return 3;
        memcpy(h, in.data(), sizeof h);
        memcpy(r, in.data() + sizeof h, sizeof r);
        const int64_t nv = h[0], nt = h[1], width = h[2], height = h[3], has_colors = h[4];
        if (in.size() != sizeof h + sizeof r + 4 * (size_t)(3 * nv + 3 * nt + (has_colors ? 3 * nv : 0))) return 3;
        const float* V = (const float*)(in.data() + sizeof h + sizeof r);
        const int32_t* T = (const int32_t*)(V + 3 * nv);
        const float* cols = has_colors ? (const float*)(T + 3 * nt) : nullptr;
        const float *cam = r + 2, *m = r + 5;
        build(M, V, T, nt);
        head(out, M, width * height);
        for (int64_t k = 0; k < width * height; k++) {
            const int j = (int)(k / width), i = (int)(k - (int64_t)j * width);
            float ray[3];
            camera_ray(cam, m, (int)width, (int)height, i, j, ray);
            const Ray R = ray_setup(cam, ray, (double)r[0], (double)r[1]);
            unsigned long long tests = 0;
            const Hit H = cast_one<false>(M, R, &tests, &out[2]);
            float dist = INFINITY, w[3] = {NAN, NAN, NAN}, rgb[3] = {0.5f, 0.75f, 1.0f};
            if (H.tri >= 0) {
                hit_outputs(H, &dist, w);
                float a[3], b[3], c[3];
                M.tris.corners((uint32_t)H.tri, a, b, c);
                const int32_t* v = T + 3 * (int64_t)H.tri;
                shade(cam, ray, dist, w, a, b, c, cols ? cols + 3 * (int64_t)v[0] : nullptr, cols ? cols + 3 * (int64_t)v[1] : nullptr,
                      cols ? cols + 3 * (int64_t)v[2] : nullptr, rgb);
            }
            out[1] += (int64_t)tests;
            out.insert(out.end(), {(int64_t)H.tri, bits(dist), bits(rgb[0]), bits(rgb[1]), bits(rgb[2]), (int64_t)tests});
        }
    } else
        return 2;
    FILE* f = fopen(argv[3], "wb");
    if (!f) return 4;
    fwrite(out.data(), sizeof(int64_t), out.size(), f);
    fclose(f);
    printf("mesh ray ok\n");
    return 0;
}
