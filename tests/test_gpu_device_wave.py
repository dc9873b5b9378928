"""The counting helpers of csrc/device_wave.h -- wave_sum, wave_add, wave_count -- in a stand-alone program built with the library's
flags: 256-lane blocks in which every lane calls them, lane i < n contributing 2^33 + i (a sum cut to 32 bits fails) and the flag
i % 3 == 0, the lanes from n on 0 / false, against the host's sums.  On the CPU: the program compiles."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5A5A5A5A5A5A5A5
# one active lane; one short of a wave, a wave, one lane into the second; one short of a block, a block, a second block with one
# active lane; several blocks with a ragged tail
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)

HARNESS = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "device_wave.h"
typedef unsigned long long u64;
// words[0]: wave_add's total; words[1]: the guard, which nothing writes
__global__ __launch_bounds__(256) void k(long n, u64* words, u64* nothing, u64* sums, unsigned* counts)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const u64 v = in ? (1ull << 33) + (u64)i : 0ull;
    wave_add(words, v);
    wave_add(nothing, v);
    const u64 s = wave_sum(v);
    const unsigned c = wave_count(in && i % 3 == 0);
    if ((threadIdx.x & 63) == 0) { sums[i >> 6] = s; counts[i >> 6] = c; }
}
int main(int argc, char** argv)
{
    for (int a = 1; a < argc; a++) {
        const long n = atol(argv[a]);
        const unsigned blocks = (unsigned)((n + 255) / 256), waves = blocks * 4;
        u64 h[2] = {0ull, 0xA5A5A5A5A5A5A5A5ull};
        u64 *words = nullptr, *sums = nullptr;
        unsigned* counts = nullptr;
        if (hipMalloc(&words, sizeof h) != hipSuccess || hipMalloc(&sums, waves * sizeof(u64)) != hipSuccess ||
            hipMalloc(&counts, waves * sizeof(unsigned)) != hipSuccess) return 3;
        if (hipMemcpy(words, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) return 3;
        hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, n, words, (u64*)nullptr, sums, counts);
        if (hipDeviceSynchronize() != hipSuccess) return 4;
        std::vector<u64> hs(waves);
        std::vector<unsigned> hc(waves);
        if (hipMemcpy(h, words, sizeof h, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hs.data(), sums, waves * sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hc.data(), counts, waves * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return 5;
        printf("%ld %llu %llu %u", n, h[0], h[1], waves);
        for (unsigned w = 0; w < waves; w++) printf(" %llu", hs[w]);
        for (unsigned w = 0; w < waves; w++) printf(" %u", hc[w]);
        printf("\n");
        if (hipFree(words) != hipSuccess || hipFree(sums) != hipSuccess || hipFree(counts) != hipSuccess) return 6;
    }
    printf("wave done\n");
    return 0;
}
"""


def _build(tmp_path):
    from sdfkit_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    (tmp_path / "w.hip").write_text(HARNESS)
    exe = str(tmp_path / "w")
    flags = [f for f in build.CFLAGS if f not in ("-fPIC", "-fvisibility=hidden")]
    subprocess.check_call([hipcc] + flags + ["-Werror", "-I", os.path.join(ROOT, "sdfkit_amd", "csrc"), str(tmp_path / "w.hip"), "-o", exe])
    return exe


def test_device_wave_program_compiles(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_device_wave_helpers_against_host_sums(gpu, tmp_path):
    exe = _build(tmp_path)
    p = subprocess.run([exe] + [str(n) for n in SIZES], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "wave done" in p.stdout, p.stdout + p.stderr
    rows = [[int(x) for x in line.split()] for line in p.stdout.splitlines()[:-1]]
    assert [r[0] for r in rows] == list(SIZES)
    for n, total, guard, waves, *rest in rows:
        assert waves == 4 * ((n + 255) // 256) and len(rest) == 2 * waves
        lanes = [range(64 * w, min(64 * w + 64, n)) for w in range(waves)]   # (empty from the first idle wave on)
        assert total == sum((1 << 33) + i for i in range(n)), n             # wave_add into a zeroed word
        assert guard == GUARD, n                                            # wave_add with a null total wrote nothing
        assert rest[:waves] == [sum((1 << 33) + i for i in r) for r in lanes], n          # wave_sum, lane 0 of every wave
        assert rest[waves:] == [sum(1 for i in r if i % 3 == 0) for r in lanes], n        # wave_count of every wave
