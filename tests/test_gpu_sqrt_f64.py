"""The device sqrt(double) the triangle-mesh distance rounds with (lib_trimesh.hip: distance = (float)sqrt(d2)) is correctly
rounded: __builtin_sqrt on binary64, built with the library's flags, against the host's IEEE sqrt on seeded random inputs over
the whole exponent range, subnormals, exact squares and the hard cases -- inputs whose square root lies next to a halfway
point between two doubles."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HARNESS = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
__global__ void k(const double* in, double* out, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __builtin_sqrt(in[i]);
}
int main(int argc, char** argv)
{
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> h;
    double x;
    while (fread(&x, 8, 1, f) == 1) h.push_back(x);
    fclose(f);
    const long n = (long)h.size();
    double *din = nullptr, *dout = nullptr;
    if (hipMalloc(&din, n * 8) != hipSuccess || hipMalloc(&dout, n * 8) != hipSuccess) return 3;
    hipMemcpy(din, h.data(), n * 8, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, din, dout, n);
    if (hipDeviceSynchronize() != hipSuccess) return 4;
    hipMemcpy(h.data(), dout, n * 8, hipMemcpyDeviceToHost);
    f = fopen(argv[2], "wb");
    fwrite(h.data(), 8, n, f);
    fclose(f);
    printf("sqrt done %ld\n", n);
    return 0;
}
"""


def _inputs():
    rng = np.random.default_rng(2024)
    bits = rng.integers(0, 0x7FF0000000000000, 200_000, dtype=np.int64)            # every finite non-negative double
    xs = [bits.view(np.float64), rng.uniform(0, 16, 100_000), rng.uniform(0, 1e-300, 1000), np.array([0.0, 5e-324, 1.0, 2.0, 3.0])]
    r = rng.uniform(0.5, 4, 20_000)
    xs.append(r * r)                                                                    # near-exact squares
    hard = []
    for m in rng.integers(1 << 52, 1 << 53, 20_000, dtype=np.int64):                    # sqrt next to a halfway point
        y = Fraction(2 * int(m) + 1, 1 << 54)
        e = int(rng.integers(-60, 60))
        hard.append(float(y * y * Fraction(2) ** (2 * e)))
    xs.append(np.array(hard))
    return np.concatenate(xs).astype(np.float64)


def test_device_sqrt_double_is_correctly_rounded(gpu, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    (tmp_path / "s.hip").write_text(HARNESS)
    exe = str(tmp_path / "s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17",
                           str(tmp_path / "s.hip"), "-o", exe], stderr=subprocess.DEVNULL)
    x = _inputs()
    x.tofile(tmp_path / "in.bin")
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "sqrt done" in p.stdout, p.stdout + p.stderr
    got = np.fromfile(tmp_path / "out.bin", np.float64)
    want = np.array([math.sqrt(v) for v in x])
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert len(bad) == 0, (len(bad), x[bad[:5]], got[bad[:5]], want[bad[:5]])
    # and what the kernels store: the binary64 root rounded to f32
    small = want < 3.0e38   # (within the f32 range)
    assert np.array_equal(got[small].astype(np.float32).view(np.uint32), want[small].astype(np.float32).view(np.uint32))
