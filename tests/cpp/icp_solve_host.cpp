// icp_solve_host.cpp -- sdfkit_amd/csrc/icp_solve.h built for the host (g++ -ffp-contract=off): the distMax rule and the filter, the
// Kabsch solve, the Matrix4x4 product and inverse and the step composition as the kernels of lib_points.hip run them, driven by
// tests/test_icp_solve.py, which compares every answer with tests/points_model.py bit for bit.  Built by hipcc with
// -DICP_SOLVE_ON_DEVICE the same cases run on the GPU instead, one lane per case (tests/test_gpu_icp_exact.py).
//
//   icp_solve_host solve  IN OUT   IN (f64): cases, then per case C (9), pmean (3), qmean (3), the previous total (16, f32 values),
//                                  converged_max_translation, converged_max_rotation
//                                  OUT (f64): per case R (9), step (16), total (16), converged (0 / 1)
//   icp_solve_host m4     IN OUT   IN (f32): cases, then per case a (16), b (16) -> OUT (f32): per case Invert(a) (16), its bool, a * b (16)
//   icp_solve_host filter IN OUT   IN (f64): cases, then per case m, sd, good, dist, mean, sqsum, n
//                                  OUT (f64): per case dist_max_rule(m, sd, good), kept(dist, that), dist_max(mean, sqsum, n, good)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#if defined(ICP_SOLVE_ON_DEVICE)
#include <hip/hip_runtime.h>
#endif

#include "../../sdfkit_amd/csrc/icp_solve.h"

using namespace sdfk_icp;

constexpr int kSolveIn = 33, kSolveOut = 42, kM4In = 32, kM4Out = 33, kFilterIn = 7, kFilterOut = 3;

SDFK_ICP_HD void solve_case(const double* in, double* out)
{
    float prev[16], step[16], total[16];
    for (int q = 0; q < 16; q++) prev[q] = (float)in[15 + q];
    bool conv;
    kabsch_r(in, out);
    solve_step(in, in + 9, in + 12, prev, (float)in[31], (float)in[32], step, total, &conv);
    for (int q = 0; q < 16; q++) { out[9 + q] = (double)step[q]; out[25 + q] = (double)total[q]; }
    out[41] = conv ? 1.0 : 0.0;
}

SDFK_ICP_HD void m4_case(const float* in, float* out)
{
    out[16] = m4_invert(in, out) ? 1.0f : 0.0f;
    m4_mul(in, in + 16, out + 17);
}

SDFK_ICP_HD void filter_case(const double* in, double* out)
{
    const float dmax = dist_max_rule((float)in[0], (float)in[1], (float)in[2]);
    out[0] = (double)dmax;
    out[1] = kept((float)in[3], dmax) ? 1.0 : 0.0;
    out[2] = (double)dist_max(in[4], in[5], in[6], (float)in[2]);
}

#if defined(ICP_SOLVE_ON_DEVICE)
template <class T, void (*F)(const T*, T*)>
__global__ void k_cases(const T* in, T* out, int cases, int nin, int nout)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < cases) F(in + (size_t)c * nin, out + (size_t)c * nout);
}
#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at line %d\n", __LINE__); exit(3); } } while (0)
#endif

template <class T, void (*F)(const T*, T*)>
static std::vector<T> run_cases(const std::vector<T>& in, int nin, int nout)
{
    const size_t cases = (size_t)in.at(0);
    if (in.size() != 1 + cases * nin) { fprintf(stderr, "bad case file\n"); exit(2); }
    std::vector<T> out(cases * nout);
    if (!cases) return out;
#if defined(ICP_SOLVE_ON_DEVICE)
    T *din = nullptr, *dout = nullptr;
    HIP_OK(hipMalloc(&din, cases * nin * sizeof(T)));
    HIP_OK(hipMalloc(&dout, out.size() * sizeof(T)));
    HIP_OK(hipMemcpy(din, in.data() + 1, cases * nin * sizeof(T), hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_cases<T, F>), dim3((unsigned)((cases + 63) / 64)), dim3(64), 0, 0, din, dout, (int)cases, nin, nout);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), dout, out.size() * sizeof(T), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(din));
    HIP_OK(hipFree(dout));
#else
    for (size_t c = 0; c < cases; c++) F(in.data() + 1 + c * nin, out.data() + c * nout);
#endif
    return out;
}

template <class T>
static std::vector<T> read_all(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)n / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("read"); exit(2); }
    fclose(f);
    return v;
}

template <class T>
static void write_all(const char* path, const std::vector<T>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const char* mode = argv[1];
    if (!strcmp(mode, "solve")) write_all(argv[3], run_cases<double, solve_case>(read_all<double>(argv[2]), kSolveIn, kSolveOut));
    else if (!strcmp(mode, "m4")) write_all(argv[3], run_cases<float, m4_case>(read_all<float>(argv[2]), kM4In, kM4Out));
    else if (!strcmp(mode, "filter")) write_all(argv[3], run_cases<double, filter_case>(read_all<double>(argv[2]), kFilterIn, kFilterOut));
    else return 2;
    printf("icp_solve_host %s ok\n", mode);
    return 0;
}
