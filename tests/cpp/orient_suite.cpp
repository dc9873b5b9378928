// orient_suite.cpp -- SdfKit::KdTree::OrientNormals (include/SdfKit.hpp) against vectors that tests/test_gpu_orient_cpp.py writes
// with the numpy model (tests/orient_model.py): every bit of every normal and every stat.  Runs on the GPU through
// libsdfkit_hip.so.
//
// File (little endian): i64 cases; per case: i64 n, k, max_seeds, stats (9: rounds, seeds, flipped, unreached, invalid, levels (4));
// static xyz (n x 3 f32); the normals given (n x 3); the model's result (n x 3).
#include <cstdio>
#include <cstring>
#include <vector>

#include "SdfKit.hpp"

using namespace SdfKit;

static int g_fail = 0, g_run = 0;
#define CHECK(cond)                                                                                     \
    do { if (!(cond)) { printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } } while (0)
#define TEST(name) static void name(); static void run_##name() { g_run++; printf("%s\n", #name); name(); } static void name()

struct Case {
    int64_t n = 0, k = 0, max_seeds = 0, stats[9] = {};
    std::vector<Vector3> P, given, want;
};
static std::vector<Case> V;

static void load(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    int64_t cases = 0;
    if (fread(&cases, sizeof cases, 1, f) != 1) { printf("short vector file\n"); exit(2); }
    V.resize((size_t)cases);
    for (Case& c : V) {
        int64_t h[12];
        if (fread(h, sizeof h, 1, f) != 1) { printf("short vector file\n"); exit(2); }
        c.n = h[0]; c.k = h[1]; c.max_seeds = h[2];
        memcpy(c.stats, h + 3, sizeof c.stats);
        for (std::vector<Vector3>* v : {&c.P, &c.given, &c.want}) {
            v->resize((size_t)c.n);
            if (fread(v->data(), sizeof(Vector3), (size_t)c.n, f) != (size_t)c.n) { printf("short vector file\n"); exit(2); }
        }
    }
    fclose(f);
}

static bool same_bits(const std::vector<Vector3>& a, const std::vector<Vector3>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(Vector3)) == 0);
}

TEST(CasesEqualTheModel)
{
    for (const Case& c : V) {
        KdTree tree(c.P);
        KdTree::OrientStats st;
        const std::vector<Vector3> got = tree.OrientNormals(c.given, (int)c.k, std::numeric_limits<float>::infinity(), (int)c.max_seeds, &st);
        CHECK(same_bits(got, c.want));
        CHECK(st.Rounds == c.stats[0] && st.Seeds == c.stats[1] && st.Flipped == c.stats[2] && st.Unreached == c.stats[3] && st.Invalid == c.stats[4]);
        for (int l = 0; l < 4; l++) CHECK(st.Levels[l] == c.stats[5 + l]);
        // applying it twice changes nothing
        CHECK(same_bits(tree.OrientNormals(got, (int)c.k, std::numeric_limits<float>::infinity(), (int)c.max_seeds), got));
    }
}

TEST(SphereComesOutOutward)
{
    const Case& c = V.at(0);   // the first case is a sphere about the origin
    KdTree tree(c.P);
    const std::vector<Vector3> got = tree.OrientNormals(c.given);
    size_t outward = 0;
    for (size_t i = 0; i < got.size(); i++) outward += got[i].X * c.P[i].X + got[i].Y * c.P[i].Y + got[i].Z * c.P[i].Z > 0 ? 1 : 0;
    CHECK(outward == got.size());
}

TEST(Refusals)
{
    const Case& c = V.at(0);
    KdTree tree(c.P);
    int refused = 0;
    try { tree.OrientNormals(c.given, 1); } catch (const std::exception&) { refused++; }
    try { tree.OrientNormals(c.given, 65); } catch (const std::exception&) { refused++; }
    try { tree.OrientNormals(c.given, 8, -1.0f); } catch (const std::exception&) { refused++; }
    try { tree.OrientNormals(c.given, 8, 1.0f, 0); } catch (const std::exception&) { refused++; }
    try { tree.OrientNormals({}); } catch (const std::exception&) { refused++; }
    CHECK(refused == 5);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: orient_suite VECTORS\n"); return 2; }
    load(argv[1]);
    run_CasesEqualTheModel(); run_SphereComesOutOutward(); run_Refusals();
    printf("%d tests, %d failures\n", g_run, g_fail);
    sdfk_shutdown();
    return g_fail ? 1 : 0;
}
