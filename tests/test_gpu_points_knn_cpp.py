"""Builds and runs tests/cpp/points_knn_suite.cpp: SdfKit::KdTree::SearchKNearest / SearchRadius of the C++ host layer
include/SdfKit.hpp against vectors written here with the numpy model (tests/points_knn_model.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import points_knn_model as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "points_knn_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "points_knn_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _vectors(path):
    rs = np.random.default_rng(21)
    P = rs.random((6000, 3), dtype=f32)
    P[100:140] = P[100]                       # duplicates
    Q = np.concatenate([rs.random((700, 3), dtype=f32), P[100:103], [[np.nan, 0, 0], [9, 9, 9]]]).astype(f32)
    k, max_distance, radius = 20, f32(0.09), f32(0.11)
    ki, kd, kf = KM.knn(P, Q, k, max_distance)
    off, ri, rd = KM.radius(P, Q, radius)
    with open(path, "wb") as f:
        f.write(struct.pack("<4q2f", len(P), len(Q), k, len(ri), max_distance, radius))
        for a in (P, Q, ki, kd, kf, off, ri, rd):
            f.write(np.ascontiguousarray(a).tobytes())
    assert (kf < k).any() and (kf == k).any() and np.diff(off).max() > 30


def test_points_knn_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the new SdfKit::KdTree methods compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_points_knn_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    _vectors(vec)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "4 tests, 0 failures" in p.stdout
