"""Builds and runs tests/cpp/points_filter_suite.cpp: SdfKit::KdTree::VoxelDownsample and RemoveStatisticalOutliers of the C++ host
layer include/SdfKit.hpp against vectors written here with the numpy model (tests/points_filter_model.py): the sphere with strays,
the merged sphere and a cloud with a voxel of many members."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import points_filter_model as FM
from tests.test_points_filter_model import recorded_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "points_filter_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "points_filter_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _clouds():
    P, _ = recorded_case()
    S = P[:2000]
    rs = np.random.default_rng(41)
    heavy = np.concatenate([FM.mixed_magnitudes(rs, 700), (rs.random((300, 3)) * 4 + 1).astype(f32)])
    return [(P, 0.25, (0, 0, 0), 8, 2.0, np.inf),
            (np.concatenate([S, (S + f32(0.001)).astype(f32)]), 0.1, (0, 0, 0), 4, 1.0, 0.05),
            (heavy, 1.0, (0.0, -0.5, 0.25), 16, 3.0, np.inf)]


def _vectors(path):
    clouds = _clouds()
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(clouds)))
        for P, size, origin, k, ratio, maxd in clouds:
            pts, cnt, group = FM.voxel_downsample(P, size, origin)
            out = FM.outliers(P, k, ratio, maxd)
            f.write(struct.pack("<10q", len(P), len(pts), k, len(out["index"]), *[int(v) for v in out["stats"]]))
            f.write(struct.pack("<6f", size, *origin, ratio, maxd))
            for a, t in ((P, f32), (pts, f32), (cnt, np.int32), (group, np.int32), (out["points"], f32), (out["index"], np.int32),
                         (out["mean_distance"], f32)):
                f.write(np.ascontiguousarray(a, t).tobytes())
    assert len(FM.voxel_downsample(*clouds[1][:3])[0]) == 1079 and FM.voxel_downsample(*clouds[2][:3])[1].max() >= 600


def test_points_filter_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the two members of SdfKit::KdTree compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_points_filter_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    _vectors(vec)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "3 tests, 0 failures" in p.stdout
