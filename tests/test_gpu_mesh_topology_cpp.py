"""Builds and runs tests/cpp/mesh_topology_suite.cpp: SdfKit::MeshSdf::Components / Topology / Select and the Mesh members of
the C++ host layer include/SdfKit.hpp against the cases recorded from the numpy model in tests/golden/mesh_topology_cases.json
(labels, rows, census and one selection per mesh).  On the CPU: the layer compiles and links."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_topology_cases as Cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32, i64 = np.float32, np.int32, np.int64


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "mesh_topology_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "mesh_topology_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _vectors(path):
    cases = Cs.load()["cases"]
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for c in cases:
            V, T = Cs.SMALL[c["mesh"]]()
            s = c["select"]
            assert (len(V), len(T)) == (c["nv"], c["nt"])
            f.write(struct.pack("<5q8q", len(V), len(T), len(c["rows"]), len(s["vertex_index"]), len(s["triangle_index"]), *c["census"]))
            f.write(np.ascontiguousarray(V, f32).tobytes() + Cs.vertex_colors(V).tobytes() + np.ascontiguousarray(T, i32).tobytes())
            f.write(np.array(c["vertex"], i32).tobytes() + np.array(c["triangle"], i32).tobytes() + np.array(c["rows"], i64).tobytes())
            f.write(np.array(s["vertex_index"], i32).tobytes() + np.array(s["triangle_index"], i32).tobytes() + np.array(s["triangles"], i32).tobytes())
    return len(cases)


def test_mesh_topology_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the members compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_mesh_topology_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    assert _vectors(vec) == len(Cs.RECORDED)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "3 tests, 0 failures" in p.stdout
