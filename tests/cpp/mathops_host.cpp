// mathops_host.cpp -- the shared arithmetic of MathF.Sin / Cos / Exp / Log / Atan2 (sdfkit_amd/csrc/mathops.h) compiled as host
// C++, for tests/test_mathops_codegen.py: the text the JIT pastes into programs, here as code, must equal the numpy model bit for bit.
//   mathops_host IN OUT
//   IN:  n pairs of float32 (a, b);  OUT: n records of 5 float32 { sin a, cos a, exp a, log a, atan2(a, b) }
#include <cstdio>
#include <vector>

#define SDFK_M_FN static inline
#define SDFK_M_TABLE static const
#define SDFK_MATHOPS_EMIT(...) __VA_ARGS__
#include "../../sdfkit_amd/csrc/mathops.h"

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    std::vector<float> ab;
    float buf[2];
    while (fread(buf, sizeof buf, 1, in) == 1) { ab.push_back(buf[0]); ab.push_back(buf[1]); }
    const size_t n = ab.size() / 2;
    std::vector<float> r(5 * n);
    for (size_t i = 0; i < n; i++) {
        const float a = ab[2 * i], b = ab[2 * i + 1];
        r[5 * i] = sdfk_sinf(a);
        r[5 * i + 1] = sdfk_cosf(a);
        r[5 * i + 2] = sdfk_expf(a);
        r[5 * i + 3] = sdfk_logf(a);
        r[5 * i + 4] = sdfk_atan2f(a, b);
    }
    fwrite(r.data(), sizeof(float), r.size(), out);
    fclose(in);
    fclose(out);
    printf("mathops ok %zu\n", n);
    return 0;
}
