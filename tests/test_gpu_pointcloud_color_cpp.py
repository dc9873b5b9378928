"""Builds and runs tests/cpp/pointcloud_color_suite.cpp: SdfKit::KdTree::SampleColors, ToVoxels and VoxelDownsample with colours of
the C++ host layer include/SdfKit.hpp against vectors written here with the numpy model (tests/pointcloud_color_model.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import pointcloud_color_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "pointcloud_color_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "pointcloud_color_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _vectors(path):
    rs = np.random.default_rng(43)
    P = rs.standard_normal((2500, 3))
    P = (P / np.linalg.norm(P, axis=1, keepdims=True)).astype(f32)       # a noisy-density sphere
    P[200:210] = P[200]                                                  # duplicates
    Nn = P.copy()
    Nn[::50] = 0
    col = (rs.standard_normal(P.shape) * 2.0 ** rs.integers(-20, 2, P.shape)).astype(f32)
    Q = np.concatenate([(rs.standard_normal((1500, 3)) * 0.7).astype(f32), P[:300], np.array([[np.nan, 0, 0]], f32)])
    k_sample, sample_distance = 12, f32(0.2)
    k_volume, shape, band, size = 8, (19, 14, 21), f32(0.3), f32(0.4)
    mn, mx = np.array([-1.4, -1.5, -0.3], f32), np.array([1.5, 1.3, 1.6], f32)
    sampled, found = CM.sample_colors(P, col, Q, k_sample, sample_distance)
    vol, known, vcol, vfound = CM.to_volume(P, Nn, col, mn, mx, shape, k_volume, band)
    pts, cnt, group, dcol = CM.voxel_downsample(P, col, size)
    with open(path, "wb") as f:
        f.write(struct.pack("<9q9f", len(P), len(Q), k_sample, k_volume, *shape, int(known.sum()), len(pts), sample_distance, band, size, *mn, *mx))
        for a, dt in ((P, f32), (col, f32), (Nn, f32), (Q, f32), (sampled, f32), (found, np.int32), (vol, f32), (vcol, f32), (pts, f32),
                      (cnt, np.int32), (group, np.int32), (dcol, f32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    assert known.any() and not known.all() and (vfound == 0).any() and (found == 0).any() and (found == k_sample).any()
    assert (cnt > 32).any() and (cnt == 1).any()


def test_pointcloud_color_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the new SdfKit::KdTree members compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_pointcloud_color_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    _vectors(vec)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "3 tests, 0 failures" in p.stdout
