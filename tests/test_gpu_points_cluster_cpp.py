"""Builds and runs tests/cpp/points_cluster_suite.cpp: SdfKit::KdTree::Clusters, SelectClusters, RemoveSmallClusters and
LargestCluster of the C++ host layer include/SdfKit.hpp against vectors written here with the numpy model
(tests/points_cluster_model.py): cloud A with and without a border, the tie and the far cloud."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import points_cluster_cases as CC
from tests import points_cluster_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "points_cluster_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "points_cluster_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _clouds():
    A, _ = CC.cloud_a()
    return [(A, 0.2, 1, 2), (A, 0.12, 10, 30), (CC.tie_clouds()[2][1], 1.0, 4, 5), (CC.far_cloud(), 0.25, 1, 3)]   # (points, radius, min_points, min_size)


def _vectors(path):
    with open(path, "wb") as f:
        clouds = _clouds()
        f.write(struct.pack("<q", len(clouds)))
        for P, radius, min_points, min_size in clouds:
            out = CM.cluster(P, radius, min_points)
            kept = CM.select(out["labels"], CM.keep_by_size(out["sizes"], min_size))
            big = np.flatnonzero(out["labels"] == CM.largest(out["sizes"])).astype(np.int32)
            f.write(struct.pack("<10q", len(P), out["n_clusters"], min_points, min_size, len(kept), len(big), *out["stats"]))
            f.write(struct.pack("<f", radius))
            for a, t in ((P, f32), (out["labels"], np.int32), (out["sizes"], np.int32), (out["core"], np.uint8), (out["counts"], np.int32),
                         (kept, np.int32), (big, np.int32)):
                f.write(np.ascontiguousarray(a, t).tobytes())
            assert 0 < len(kept) < len(P) and len(big) > 0


def test_points_cluster_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the four members of SdfKit::KdTree compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_points_cluster_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    _vectors(vec)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "3 tests, 0 failures" in p.stdout
