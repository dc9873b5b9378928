// interval_host.cpp -- the SHIPPED text of SDF programs (what the code generator emits before `#define SDFK_WRITES_COLOR`: the
// preludes, struct SdfkK, sdf_eval, sdf_interval) built as plain host C++ behind tests/cpp/interval_shim.h, for
// tests/test_interval_codegen.py: sdf_interval over boxes and sdf_eval at points, program by program.
//   g++ -O2 -ffp-contract=off -DSDFK_KERNELS=0x200 -DINTERVAL_PROGRAMS='"programs.inc"' [-DINTERVAL_HAS_VOLUMES] interval_host.cpp
// programs.inc is written by the test: the preludes once, then per program
//   namespace pN { <struct SdfkK .. sdf_interval of the generated source> INTERVAL_RUN(n_params, <K.V = V; or nothing>) }
// and `static const interval_run_fn kPrograms[] = {p0::run, ...};`.
//   interval_host IN OUT        IN: records { int32 program, nk, nvol, nbox, npt; float k[nk]; nvol volumes; float box[nbox][6]
//                               (x lo, x hi, y lo, y hi, z lo, z hi); float pt[npt][3] }
//                               a volume: { int32 n[3], pitch, has_colors, nlev; float mn[3], d[3], m[3]; float val[n0 n1 pitch];
//                               float col[3 n0 n1 pitch] if has_colors; per channel 0..3 (0..2 only with colours): per level 1..nlev
//                               { int32 cells; float lohi[2 cells] } }
//                               OUT: per record float iv[nbox][2], float w[npt]
//   interval_host IN OUT sqrt   IN: floats; OUT: sdfk_sqrt of each
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "interval_shim.h"

struct SdfkVolHost;
typedef void (*interval_run_fn)(const float* k, const void* V, int nbox, const float* b, float* iv, int npt, const float* p, float* w);
#define INTERVAL_RUN(NK, SETV)                                                                                                  \
    static void run(const float* k, const void* V, int nbox, const float* b, float* iv, int npt, const float* p, float* w)      \
    {                                                                                                                           \
        SdfkK K;                                                                                                                \
        memset(&K, 0, sizeof K);                                                                                                \
        for (int i = 0; i < NK; i++) K.k[i] = k[i];                                                                             \
        (void)V;                                                                                                                \
        SETV                                                                                                                    \
        for (int i = 0; i < nbox; i++) {                                                                                        \
            sdfk_iv X, Y, Z;                                                                                                    \
            X.lo = b[6 * i]; X.hi = b[6 * i + 1]; Y.lo = b[6 * i + 2]; Y.hi = b[6 * i + 3]; Z.lo = b[6 * i + 4]; Z.hi = b[6 * i + 5]; \
            const sdfk_iv r = sdf_interval(K, X, Y, Z);                                                                         \
            iv[2 * i] = r.lo; iv[2 * i + 1] = r.hi;                                                                             \
        }                                                                                                                       \
        for (int i = 0; i < npt; i++) {                                                                                         \
            float R, G, B, W;                                                                                                   \
            sdf_eval(K, p[3 * i], p[3 * i + 1], p[3 * i + 2], R, G, B, W);                                                      \
            w[i] = W;                                                                                                           \
        }                                                                                                                       \
    }

#include INTERVAL_PROGRAMS

static FILE* g_in;
template <class T> static std::vector<T> rd(size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, g_in) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s IN OUT [sqrt]\n", argv[0]); return 2; }
    g_in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!g_in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    if (argc > 3) {
        fseek(g_in, 0, SEEK_END);
        const long n = ftell(g_in) / 4;
        fseek(g_in, 0, SEEK_SET);
        std::vector<float> x = rd<float>((size_t)n);
        for (float& v : x) v = sdfk_sqrt(v);
        fwrite(x.data(), 4, x.size(), out);
        fclose(out);
        printf("interval ok %ld\n", n);
        return 0;
    }
    const int nprog = (int)(sizeof kPrograms / sizeof kPrograms[0]);
    int n = 0;
    for (;;) {
        int32_t h[5];
        if (fread(h, sizeof h, 1, g_in) != 1) break;
        if (h[0] < 0 || h[0] >= nprog) { fprintf(stderr, "no program %d\n", h[0]); return 2; }
        std::vector<float> k = rd<float>((size_t)h[1]);
        std::vector<std::vector<float>> keep;   // the volumes' arrays (the descriptors point into them)
        const void* table = nullptr;
#ifdef INTERVAL_HAS_VOLUMES
        std::vector<SdfkVol> vols((size_t)h[2]);
        for (SdfkVol& V : vols) {
            memset(&V, 0, sizeof V);
            std::vector<int32_t> q = rd<int32_t>(6);
            for (int a = 0; a < 3; a++) V.n[a] = q[a];
            V.pitch = q[3];
            V.nlev = q[5];
            std::vector<float> g = rd<float>(9);
            for (int a = 0; a < 3; a++) { V.mn[a] = g[a]; V.d[a] = g[3 + a]; V.m[a] = g[6 + a]; }
            const size_t cells = (size_t)q[0] * q[1] * q[3];
            keep.push_back(rd<float>(cells));
            V.val = keep.back().data();
            if (q[4]) { keep.push_back(rd<float>(3 * cells)); V.col = keep.back().data(); }
            for (int ch = q[4] ? 0 : 3; ch < 4; ch++) {
                std::vector<float> all(2, 0.0f);   // (level L at cell offset lev[L]; offset 0 is never a level's)
                for (int L = 1; L <= q[5]; L++) {
                    const int32_t c = rd<int32_t>(1)[0];
                    std::vector<float> lohi = rd<float>(2 * (size_t)c);
                    V.lev[L] = (long long)(all.size() / 2);
                    all.insert(all.end(), lohi.begin(), lohi.end());
                }
                keep.push_back(all);
                V.pyr[ch] = keep.back().data();
            }
        }
        table = vols.data();
#else
        if (h[2]) { fprintf(stderr, "built without volumes\n"); return 2; }
#endif
        std::vector<float> b = rd<float>(6 * (size_t)h[3]), p = rd<float>(3 * (size_t)h[4]);
        std::vector<float> iv(2 * (size_t)h[3]), w((size_t)h[4]);
        kPrograms[h[0]](k.data(), table, h[3], b.data(), iv.data(), h[4], p.data(), w.data());
        fwrite(iv.data(), 4, iv.size(), out);
        fwrite(w.data(), 4, w.size(), out);
        n++;
    }
    fclose(out);
    printf("interval ok %d\n", n);
    return 0;
}
