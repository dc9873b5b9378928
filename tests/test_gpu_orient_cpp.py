"""Builds and runs tests/cpp/orient_suite.cpp: SdfKit::KdTree::OrientNormals of the C++ host layer include/SdfKit.hpp against
vectors written here with the numpy model (tests/orient_model.py): the sphere and the two-cluster case."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import orient_cases as OC
from tests import orient_model as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "orient_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "orient_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _vectors(path):
    cases = [("sphere", 8, 64), ("two_spheres", 8, 64), ("two_spheres", 8, 1)]
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for name, k, max_seeds in cases:
            P, _, nrm = OC.cloud(name)
            want, st = OM.orient(P, nrm, k, max_seeds=max_seeds)
            f.write(struct.pack("<12q", len(P), k, max_seeds, st["rounds"], st["seeds"], st["flipped"], st["unreached"], st["invalid"], *st["levels"]))
            for a in (P, nrm, want):
                f.write(np.ascontiguousarray(a, f32).tobytes())
            assert st["seeds"] == min(max_seeds, 2 if name == "two_spheres" else 1) and (st["unreached"] > 0) == (max_seeds == 1 and name == "two_spheres")


def test_orient_cpp_host_layer_compiles(tmp_path):
    """CPU-side: SdfKit::KdTree::OrientNormals compiles and links against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_orient_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    _vectors(vec)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "3 tests, 0 failures" in p.stdout
