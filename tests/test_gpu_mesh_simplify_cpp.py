"""Builds and runs tests/cpp/mesh_simplify_suite.cpp: SdfKit::MeshSdf::Simplify and Mesh::Simplify of the C++ host layer
include/SdfKit.hpp against the cases recorded from the numpy model in tests/golden/mesh_simplify_cases.json (every output under
every placement and duplicate rule, as integers and bits).  On the CPU: the layer compiles and links."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_simplify_cases as Cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32, u32 = np.float32, np.int32, np.uint32


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "mesh_simplify_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "mesh_simplify_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _vectors(path):
    cases = Cs.load()["cases"]
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for c in cases:
            V, T, cols, cell = Cs.SMALL[c["mesh"]]()
            assert (len(V), len(T), cols is not None, float(f32(cell))) == (c["nv"], c["nt"], c["colors"], c["cell"])
            assert len(c["runs"]) == len(Cs.PLACEMENTS) * len(Cs.FLAGS)
            f.write(struct.pack("<4q2f", len(V), len(T), int(cols is not None), len(c["runs"]), cell, 0.0))
            f.write(np.ascontiguousarray(V, f32).tobytes() + np.ascontiguousarray(T, i32).tobytes())
            if cols is not None:
                f.write(np.ascontiguousarray(cols, f32).tobytes())
            for w in c["runs"]:
                f.write(struct.pack("<10q", w["placement"], w["flags"], len(w["vertex_index"]), len(w["triangle_index"]), *w["stats"]))
                for key in ("vertex_index", "triangle_index", "triangles"):
                    f.write(np.array(w[key], i32).tobytes())
                for key in ("vertices", "colors"):
                    f.write(np.array(w[key], u32).tobytes())
    return len(cases)


def test_mesh_simplify_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the members compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_mesh_simplify_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    assert _vectors(vec) == len(Cs.RECORDED)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "3 tests, 0 failures" in p.stdout
