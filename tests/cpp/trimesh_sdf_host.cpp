// trimesh_sdf_host.cpp -- the arithmetic of the triangle-mesh distance (sdfkit_amd/csrc/trimesh_sdf.h, compiled here as plain C++
// with -ffp-contract=off, the functions the kernels call) on cases written by tests/test_trimesh_sdf_host.py, whose results
// that test compares bit for bit with the numpy model (tests/meshsdf_model.py).
//   trimesh_sdf_host closest IN OUT   IN: n x 12 float32 (p, a, b, c)     OUT: n x 7 float64 (d2, cp[3], w[3])
//   trimesh_sdf_host orient IN OUT    IN: n x 6 float32 (a, b, p in xy)   OUT: n x 2 int32 (exact sign, perturbed sign)
//   trimesh_sdf_host column IN OUT    IN: n x 11 float32 (a, b, c, px, py) OUT: n x 2 float64 (area * 2 + inside, z_cross)
//   trimesh_sdf_host colrange IN OUT  IN: n x 5 float32 (lo, hi, m, d, count) OUT: n x 2 int32 (i0, i1 of col_range)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/trimesh_sdf.h"

using namespace sdfk_trimesh_sdf;

template <typename T>
static std::vector<T> read_all(const char* path)
{
    std::vector<T> v;
    FILE* f = fopen(path, "rb");
    if (!f) return v;
    T x;
    while (fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    fclose(f);
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s closest|orient|column|colrange IN OUT\n", argv[0]); return 2; }
    const std::vector<float> in = read_all<float>(argv[2]);
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 2;
    if (!strcmp(argv[1], "closest")) {
        for (size_t i = 0; i + 12 <= in.size(); i += 12) {
            const double p[3] = {in[i], in[i + 1], in[i + 2]}, a[3] = {in[i + 3], in[i + 4], in[i + 5]};
            const double b[3] = {in[i + 6], in[i + 7], in[i + 8]}, c[3] = {in[i + 9], in[i + 10], in[i + 11]};
            const Closest R = closest_on_triangle(p, a, b, c);
            const double o[7] = {R.d2, R.cp[0], R.cp[1], R.cp[2], R.w[0], R.w[1], R.w[2]};
            fwrite(o, sizeof o, 1, out);
        }
    } else if (!strcmp(argv[1], "orient")) {
        for (size_t i = 0; i + 6 <= in.size(); i += 6) {
            const int32_t o[2] = {orient2d_exact(in[i], in[i + 1], in[i + 2], in[i + 3], in[i + 4], in[i + 5]),
                                  orient2d_perturbed(in[i], in[i + 1], in[i + 2], in[i + 3], in[i + 4], in[i + 5])};
            fwrite(o, sizeof o, 1, out);
        }
    } else if (!strcmp(argv[1], "column")) {
        for (size_t i = 0; i + 11 <= in.size(); i += 11) {
            const float a[3] = {in[i], in[i + 1], in[i + 2]}, b[3] = {in[i + 3], in[i + 4], in[i + 5]}, c[3] = {in[i + 6], in[i + 7], in[i + 8]};
            const int area = projected_area_sign(a, b, c);
            const bool inside = area != 0 && column_inside(a, b, c, area, in[i + 9], in[i + 10]);
            const double o[2] = {(double)(area * 2 + (inside ? 1 : 0)), area != 0 ? z_cross(a, b, c, area, in[i + 9], in[i + 10]) : 0.0};
            fwrite(o, sizeof o, 1, out);
        }
    } else if (!strcmp(argv[1], "colrange")) {
        for (size_t i = 0; i + 5 <= in.size(); i += 5) {
            int32_t o[2];
            col_range(in[i], in[i + 1], in[i + 2], in[i + 3], (int)in[i + 4], &o[0], &o[1]);
            fwrite(o, sizeof o, 1, out);
        }
    } else {
        fclose(out);
        return 2;
    }
    fclose(out);
    printf("trimesh ok\n");
    return 0;
}
