"""The bit logic of the count pass that reads the sampler's sign BYTES (k_count_bytes, csrc/mc_signbytes.h), on the host: the 8 x 8 byte
transposition in registers, the next-word bits, and a lane-by-lane walk of a wavefront's column against what the two kernels it
replaces compute -- the words as k_bits_transpose regroups them, segment_mask on those words as k_compact walks them: transposed
words, masks, counts, case-13 counts and validity bits, bit for bit.  tests/cpp/signbytes_host.cpp is a stand-alone program (its own
main) that includes the very header the kernel includes; all-zero, all-one, checkerboards, random fills, a single set / clear bit at
every byte and bit position, nx = 64, 65, 72, 128, ny = 2, 3, rows with padding, a 512-layer chunk boundary.  It is built and run twice:
plainly, and with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "signbytes_host.cpp")


@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")], ids=["plain", "asan_ubsan"])
def test_signbytes_host_program(tmp_path, flags):
    exe = str(tmp_path / "signbytes_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *flags, SRC, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    last = p.stdout.strip().splitlines()[-1]
    assert last.startswith("signbytes_host:") and last.endswith(" 0 failed"), last
    assert int(last.split()[1]) > 1_000_000   # (it did check something)
