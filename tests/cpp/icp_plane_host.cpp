// icp_plane_host.cpp -- the point-to-plane part of sdfkit_amd/csrc/icp_solve.h built for the host (g++ -ffp-contract=off): plane_row,
// jacobi6 / pinv_solve6, cayley_step and solve_step_plane as the kernels of lib_points.hip run them, driven by
// tests/test_icp_plane_solve.py, which compares every answer with tests/icp_plane_model.py bit for bit.
//
//   icp_plane_host row   IN OUT   IN (f64): cases, then per case p (3), q (3), n (3) (f32 values), pmean (3)
//                                 OUT (f64): per case J (6), r
//   icp_plane_host solve IN OUT   IN (f64): cases, then per case A (21: the upper triangle in row order), b (6), pmean (3), the previous
//                                 total (16, f32 values), converged_max_translation, converged_max_rotation
//                                 OUT (f64): per case lambda (6), x (6), retained, R (9), T (3), step (16), total (16), converged (0 / 1)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sdfkit_amd/csrc/icp_solve.h"

using namespace sdfk_icp;

constexpr int kRowIn = 12, kRowOut = 7, kSolveIn = 48, kSolveOut = 58;

static void row_case(const double* in, double* out)
{
    float p[3], q[3], n[3];
    for (int a = 0; a < 3; a++) { p[a] = (float)in[a]; q[a] = (float)in[3 + a]; n[a] = (float)in[6 + a]; }
    plane_row(p, q, n, in + 9, out, out + 6);
}

static void solve_case(const double* in, double* out)
{
    float prev[16], step[16], total[16];
    for (int q = 0; q < 16; q++) prev[q] = (float)in[30 + q];
    bool conv;
    int retained;
    pinv_solve6(in, in + 21, out + 6, out);
    cayley_step(out + 6, in + 27, out + 13, out + 22);
    solve_step_plane(in, in + 21, in + 27, prev, (float)in[46], (float)in[47], step, total, &conv, &retained);
    out[12] = (double)retained;
    for (int q = 0; q < 16; q++) { out[25 + q] = (double)step[q]; out[41 + q] = (double)total[q]; }
    out[57] = conv ? 1.0 : 0.0;
}

static std::vector<double> run_cases(const std::vector<double>& in, int nin, int nout, void (*f)(const double*, double*))
{
    const size_t cases = (size_t)in.at(0);
    if (in.size() != 1 + cases * nin) { fprintf(stderr, "bad case file\n"); exit(2); }
    std::vector<double> out(cases * nout);
    for (size_t c = 0; c < cases; c++) f(in.data() + 1 + c * nin, out.data() + c * nout);
    return out;
}

static std::vector<double> read_all(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<double> v((size_t)n / sizeof(double));
    if (fread(v.data(), sizeof(double), v.size(), f) != v.size()) { perror("read"); exit(2); }
    fclose(f);
    return v;
}

static void write_all(const char* path, const std::vector<double>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const char* mode = argv[1];
    if (!strcmp(mode, "row")) write_all(argv[3], run_cases(read_all(argv[2]), kRowIn, kRowOut, row_case));
    else if (!strcmp(mode, "solve")) write_all(argv[3], run_cases(read_all(argv[2]), kSolveIn, kSolveOut, solve_case));
    else return 2;
    printf("icp_plane_host %s ok\n", mode);
    return 0;
}
