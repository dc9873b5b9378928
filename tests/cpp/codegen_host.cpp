// codegen_host.cpp -- the SDF code generator (sdfkit_amd/csrc/sample_codegen.h) built as plain host C++, for
// tests/test_voxel_sdf_codegen.py: it writes the generated HIP source of every program in IN, so that the test can pin the
// source of volume-less programs byte for byte and look at the source of programs that read bound volumes.
//   codegen_host IN OUT
//   IN:  per program { int32 n_ops, out_rgbw[4], writes_color, n_volumes; n_ops x { int32 opcode, a, b, c, d; float imm } }
//   OUT: per program { int32 status (1 = generated), int32 length; length bytes of source (or of the error message) }
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sdfkit_amd/csrc/sample_codegen.h"

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    int n = 0;
    for (;;) {
        int32_t hdr[7];
        if (fread(hdr, sizeof hdr, 1, in) != 1) break;
        std::vector<sdfk_op> ops((size_t)hdr[0]);
        if (hdr[0] > 0 && fread(ops.data(), sizeof(sdfk_op), ops.size(), in) != ops.size()) { fprintf(stderr, "short read\n"); return 2; }
        std::string src, err;
        const bool ok = sdfk::generate_sample_source(ops.data(), hdr[0], hdr + 1, hdr[5], src, err, nullptr, hdr[6]);
        const std::string& text = ok ? src : err;
        const int32_t rec[2] = {ok ? 1 : 0, (int32_t)text.size()};
        fwrite(rec, sizeof rec, 1, out);
        fwrite(text.data(), 1, text.size(), out);
        n++;
    }
    fclose(in);
    fclose(out);
    printf("codegen ok %d\n", n);
    return 0;
}
