"""Builds and runs tests/cpp/icp_plane_suite.cpp: the point-to-plane members of SdfKit::IterativeClosestPoint (include/SdfKit.hpp)
reproduce the C ABI's total, points, iteration count and stats on a height-field case, and keep StaticNormals in step."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "icp_plane_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "icp_plane_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_icp_plane_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the new members compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_icp_plane_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "2 tests, 0 failures" in p.stdout
