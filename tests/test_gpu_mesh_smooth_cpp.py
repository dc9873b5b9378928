"""Builds and runs tests/cpp/mesh_smooth_suite.cpp: SdfKit::MeshSdf::Adjacency / Smooth / VertexNormals and Mesh::Smooth /
RecomputeNormals of the C++ host layer include/SdfKit.hpp against the cases recorded from the numpy model in
tests/golden/mesh_smooth_cases.json (adjacency, smoothed positions, normals, bit for bit).  On the CPU: the layer compiles and
links."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_smooth_cases as Cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32, u32, u8 = np.float32, np.int32, np.uint32, np.uint8


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "mesh_smooth_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "mesh_smooth_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _vectors(path):
    doc = Cs.load()
    cases = doc["cases"]
    with open(path, "wb") as f:
        f.write(struct.pack("<2q2f", len(cases), doc["iterations"], doc["lambda"], doc["mu"]))
        for c in cases:
            V, T = Cs.SMALL[c["mesh"]]()
            assert (len(V), len(T)) == (c["nv"], c["nt"])
            f.write(struct.pack("<3q", len(V), len(T), len(c["neighbors"])))
            f.write(np.ascontiguousarray(V, f32).tobytes() + np.ascontiguousarray(T, i32).tobytes())
            f.write(np.array(c["start"], u32).tobytes() + np.array(c["neighbors"], u32).tobytes() + np.array(c["boundary"], u8).tobytes())
            for key in ("smoothed", "normals", "smoothed_normals_flipped"):
                f.write(np.array(c[key], u32).tobytes())
    return len(cases)


def test_mesh_smooth_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the members compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_mesh_smooth_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    assert _vectors(vec) == len(Cs.RECORDED)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "3 tests, 0 failures" in p.stdout
