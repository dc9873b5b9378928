"""Builds and runs tests/cpp/pointcloud_suite.cpp: SdfKit::KdTree::EstimateNormals / ToVoxels of the C++ host layer
include/SdfKit.hpp against vectors written here with the numpy model (tests/pointcloud_model.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import pointcloud_model as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "pointcloud_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "pointcloud_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _vectors(path):
    rs = np.random.default_rng(41)
    P = rs.standard_normal((2500, 3))
    P = (P / np.linalg.norm(P, axis=1, keepdims=True)).astype(f32)       # a noisy-density sphere
    P[200:210] = P[200]                                                  # duplicates
    view = np.array([0.25, -0.5, 4.0], f32)
    k_normals, k_volume, shape, band = 12, 8, (19, 14, 21), f32(0.3)
    mn, mx = np.array([-1.4, -1.5, -0.3], f32), np.array([1.5, 1.3, 1.6], f32)
    nrm, var = PC.normals(P, k_normals, view)
    vol_normals = P.copy()
    vol, known = PC.to_volume(P, vol_normals, mn, mx, shape, k_volume, band)
    with open(path, "wb") as f:
        f.write(struct.pack("<7q10f", len(P), k_normals, k_volume, *shape, int(known.sum()), band, *view, *mn, *mx))
        for a in (P, nrm, var, vol_normals, vol):
            f.write(np.ascontiguousarray(a, f32).tobytes())
    assert known.any() and not known.all()


def test_pointcloud_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the new SdfKit::KdTree methods compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_pointcloud_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    _vectors(vec)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "3 tests, 0 failures" in p.stdout
