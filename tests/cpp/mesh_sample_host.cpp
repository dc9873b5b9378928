// mesh_sample_host.cpp -- the arithmetic of mesh sampling (sdfkit_amd/csrc/trimesh_sample.h, compiled here as plain C++ with
// -ffp-contract=off, the functions the kernels call) on cases written by tests/test_mesh_sample_host.py, whose results that test
// compares bit for bit with the numpy model (tests/mesh_sample_model.py).
//   mesh_sample_host area IN OUT     IN: n x 9 float32 (a, b, c)                     OUT: n x 4 float64 (n[3], A2)
//   mesh_sample_host weight IN OUT   IN: n x 2 float64 (A2, A2max)                   OUT: n uint64
//   mesh_sample_host draw IN OUT     IN: n x 2 uint64 (seed, s)                      OUT: n x 3 uint64 (h0, h1, h2)
//   mesh_sample_host pick IN OUT     IN: n x 5 uint64 (h0, s, n, total, stratified)  OUT: n uint64 (r)
//   mesh_sample_host find IN OUT     IN: uint64 nt, W[nt + 1], then the r            OUT: int64 per r
//   mesh_sample_host sample IN OUT   IN: n x {float32 tri[9], pad; uint64 h1, h2}    OUT: n x {float32 point[3], normal[3], weights[3], pad; float64 w[3]}
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/trimesh_sample.h"

using namespace sdfk_trimesh_smp;

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

struct SampleIn { float tri[9]; float pad; uint64_t h[2]; };
struct SampleOut { float o[9]; float pad; double w[3]; };

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s area|weight|draw|pick|find|sample IN OUT\n", argv[0]); return 2; }
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 2;
    if (!strcmp(argv[1], "area")) {
        const std::vector<float> in = read_all<float>(argv[2]);
        for (size_t i = 0; i + 9 <= in.size(); i += 9) {
            double o[4];
            o[3] = area2(&in[i], &in[i + 3], &in[i + 6], o);
            fwrite(o, sizeof o, 1, out);
        }
    } else if (!strcmp(argv[1], "weight")) {
        const std::vector<double> in = read_all<double>(argv[2]);
        for (size_t i = 0; i + 2 <= in.size(); i += 2) {
            const uint64_t o = weight(in[i], in[i + 1]);
            fwrite(&o, sizeof o, 1, out);
        }
    } else if (!strcmp(argv[1], "draw")) {
        const std::vector<uint64_t> in = read_all<uint64_t>(argv[2]);
        for (size_t i = 0; i + 2 <= in.size(); i += 2) {
            const uint64_t o[3] = {draw(in[i], in[i + 1], 0), draw(in[i], in[i + 1], 1), draw(in[i], in[i + 1], 2)};
            fwrite(o, sizeof o, 1, out);
        }
    } else if (!strcmp(argv[1], "pick")) {
        const std::vector<uint64_t> in = read_all<uint64_t>(argv[2]);
        for (size_t i = 0; i + 5 <= in.size(); i += 5) {
            const uint64_t o = pick(in[i], in[i + 1], in[i + 2], in[i + 3], in[i + 4] != 0);
            fwrite(&o, sizeof o, 1, out);
        }
    } else if (!strcmp(argv[1], "find")) {
        const std::vector<unsigned long long> in = read_all<unsigned long long>(argv[2]);
        if (in.empty() || in.size() < in[0] + 2) { fclose(out); return 2; }
        const int64_t nt = (int64_t)in[0];
        for (size_t i = (size_t)nt + 2; i < in.size(); i++) {
            const int64_t o = find_triangle(&in[1], nt, in[i]);
            fwrite(&o, sizeof o, 1, out);
        }
    } else if (!strcmp(argv[1], "sample")) {
        const std::vector<SampleIn> in = read_all<SampleIn>(argv[2]);
        for (const SampleIn& r : in) {
            const Sample S = sample_on(r.tri, r.tri + 3, r.tri + 6, r.h[0], r.h[1]);
            SampleOut o{};
            for (int k = 0; k < 3; k++) { o.o[k] = S.point[k]; o.o[3 + k] = S.normal[k]; o.o[6 + k] = S.weights[k]; o.w[k] = S.w[k]; }
            fwrite(&o, sizeof o, 1, out);
        }
    } else {
        fclose(out);
        return 2;
    }
    fclose(out);
    printf("mesh sample ok\n");
    return 0;
}
