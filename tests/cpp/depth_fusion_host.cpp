// depth_fusion_host.cpp -- the per-voxel and per-pixel functions of sdfkit_amd/csrc/depth_fusion.h (the very code the kernels of
// lib_fusion.hip run) looped over a case on the CPU: tests/test_depth_fusion_host.py holds the results to the numpy model bit for bit.
//   depth_fusion_host integrate IN OUT   one frame into a volume: IN = int64 nx, ny, nz, nz_global, z0, width, height, flags; f32
//       truncation, depth_min, depth_max, weight, max_weight; min[3], max[3], cam[3], m[16]; depth; D; W.  OUT = int64 stats[4]; D'; W'.
//   depth_fusion_host unproject IN OUT   IN = int64 width, height, has_rgb; f32 depth_min, depth_max; cam[3], m[16]; depth; rgb.
//       OUT = int64 n; points[3 n]; colors[3 n] (with rgb); int32 pixel[n].
//   depth_fusion_host refusals IN OUT    IN = records of f32 truncation, depth_min, depth_max, weight, max_weight; int32 flags, width,
//       height; two volumes of int32 nx, ny, nz, nz_global, z0; f32 min[3], max[3]; int32 storage.  OUT = a line per record: the
//       refusal, or nothing.
// Build: g++ -std=c++17 -O2 -ffp-contract=off (and once more with -fsanitize=address,undefined).
#include "../../sdfkit_amd/csrc/depth_fusion.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace sdfk_depth_fusion;

static std::vector<char> read_file(const char* path)
{
    std::vector<char> b;
    FILE* f = fopen(path, "rb");
    if (!f) return b;
    char tmp[1 << 16];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) b.insert(b.end(), tmp, tmp + n);
    fclose(f);
    return b;
}

struct Reader {
    const std::vector<char>& b;
    size_t at = 0;
    bool ok = true;
    template <class T>
    void get(T* out, size_t count)
    {
        const size_t bytes = count * sizeof(T);
        if (!ok || at + bytes > b.size()) { ok = false; return; }
        if (bytes) memcpy(out, b.data() + at, bytes);
        at += bytes;
    }
};

template <class T>
static void put(std::vector<char>& out, const T* p, size_t count)
{
    const char* c = (const char*)p;
    out.insert(out.end(), c, c + count * sizeof(T));
}

static int integrate(Reader& in, std::vector<char>& out)
{
    int64_t h[8];
    float prm[5], mn[3], mx[3];
    Frame F;
    in.get(h, 8); in.get(prm, 5); in.get(mn, 3); in.get(mx, 3); in.get(F.cam, 3); in.get(F.m, 16);
    if (!in.ok) return 2;
    const int nx = (int)h[0], ny = (int)h[1], nz = (int)h[2], nzg = (int)h[3], z0 = (int)h[4];
    F.width = (int)h[5]; F.height = (int)h[6];
    const Params P{prm[0], prm[1], prm[2], prm[3], prm[4], (int)h[7] & 1};
    const size_t nvox = (size_t)nx * ny * nz, npix = (size_t)F.width * F.height;
    std::vector<float> depth(npix), D(nvox), W(nvox);
    in.get(depth.data(), npix); in.get(D.data(), nvox); in.get(W.data(), nvox);
    if (!in.ok) return 2;
    // the library's grid constants (lib_volume.hip, grid_constants): cell size, first centre
    const int n[3] = {nx, ny, nzg};
    float d[3], m[3];
    for (int a = 0; a < 3; a++) {
        d[a] = (mx[a] - mn[a]) / (float)n[a];
        const float half = 0.5f * d[a];
        m[a] = mn[a] + half;
    }
    int64_t stats[4] = {0, 0, 0, 0};
    for (int i = 0; i < nx; i++)
        for (int j = 0; j < ny; j++)
            for (int k = 0; k < nz; k++) {
                const float p[3] = {centre(m[0], i, d[0]), centre(m[1], j, d[1]), centre(m[2], z0 + k, d[2])};
                int64_t pixel;
                if (!project(F, p, &pixel)) continue;
                if (pixel < 0 || pixel >= (int64_t)npix) return 3;   // (never: the range was decided in float)
                float t;
                const Kind kind = classify(F, P, p, depth[(size_t)pixel], &t);
                if (kind == SKIP) continue;
                const size_t v = ((size_t)i * ny + j) * nz + k;
                float D1, W1;
                const bool first = update(P, t, D[v], W[v], &D1, &W1);
                D[v] = D1; W[v] = W1;
                stats[0]++;
                stats[1] += kind == SURFACE;
                stats[2] += first;
            }
    for (size_t k = 0; k < npix; k++) stats[3] += depth_valid(depth[k], P.depth_min, P.depth_max);
    put(out, stats, 4); put(out, D.data(), nvox); put(out, W.data(), nvox);
    return 0;
}

static int unproject_frame(Reader& in, std::vector<char>& out)
{
    int64_t h[3];
    float range[2], cam[3], m[16];
    in.get(h, 3); in.get(range, 2); in.get(cam, 3); in.get(m, 16);
    if (!in.ok) return 2;
    const int width = (int)h[0], height = (int)h[1];
    const size_t npix = (size_t)width * height;
    std::vector<float> depth(npix), rgb(h[2] ? 3 * npix : 0), pts, cols;
    std::vector<int32_t> pix;
    in.get(depth.data(), npix); in.get(rgb.data(), rgb.size());
    if (!in.ok) return 2;
    for (int j = 0; j < height; j++)
        for (int i = 0; i < width; i++) {
            const size_t k = (size_t)j * width + i;
            if (!depth_valid(depth[k], range[0], range[1])) continue;
            float p[3];
            unproject(cam, m, width, height, i, j, depth[k], p);
            pts.insert(pts.end(), p, p + 3);
            if (h[2]) cols.insert(cols.end(), rgb.begin() + 3 * k, rgb.begin() + 3 * k + 3);
            pix.push_back((int32_t)k);
        }
    const int64_t n = (int64_t)pix.size();
    put(out, &n, 1); put(out, pts.data(), pts.size()); put(out, cols.data(), cols.size()); put(out, pix.data(), pix.size());
    return 0;
}

static int refusals(Reader& in, std::vector<char>& out)
{
    while (in.at < in.b.size()) {
        float prm[5];
        int32_t q[3];
        VolumeShape v[2];
        in.get(prm, 5); in.get(q, 3);
        for (int s = 0; s < 2; s++) {
            int32_t dims[5], storage;
            in.get(dims, 5); in.get(v[s].gmin, 3); in.get(v[s].gmax, 3); in.get(&storage, 1);
            v[s].nx = dims[0]; v[s].ny = dims[1]; v[s].nz = dims[2]; v[s].nz_global = dims[3]; v[s].z0 = dims[4];
            v[s].storage = storage != 0;
        }
        if (!in.ok) return 2;
        const char* e = volumes_refusal(v[0], v[1]);
        if (!e) e = image_refusal(q[1], q[2]);
        if (!e) e = params_refusal(prm[0], prm[1], prm[2], prm[3], prm[4], q[0]);
        const std::string line = std::string(e ? e : "") + "\n";
        put(out, line.data(), line.size());
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 1;
    const std::vector<char> blob = read_file(argv[2]);
    Reader in{blob};
    std::vector<char> out;
    const std::string mode = argv[1];
    const int r = mode == "integrate" ? integrate(in, out) : mode == "unproject" ? unproject_frame(in, out) : mode == "refusals" ? refusals(in, out) : 1;
    if (r) return r;
    FILE* f = fopen(argv[3], "wb");
    if (!f) return 4;
    if (!out.empty() && fwrite(out.data(), 1, out.size(), f) != out.size()) return 4;
    fclose(f);
    printf("depth fusion ok\n");
    return 0;
}
