"""Builds and runs tests/cpp/mesh_sample_suite.cpp: SdfKit::MeshSdf::SamplePoints / Mesh::SamplePoints of the C++ host layer
include/SdfKit.hpp against the cases recorded from the numpy model in tests/golden/mesh_sample_cases.json (the first 32 samples
of every output as bits, a hash of all of them, the stats).  On the CPU: the layer compiles and links, and the model still
reproduces the recorded cases."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_sample_cases as Cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MESHES = {"box": Cs.box, "weight_quantisation": Cs.weight_quantisation, "sheet": Cs.sheet}


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "mesh_sample_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "mesh_sample_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _bits(words):
    return np.array(words, np.uint32).view(f32)


def _vectors(path):
    cases = Cs.load()["cases"]
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for c in cases:
            V, T = MESHES[c["mesh"]]()
            k = len(c["triangles"])
            f.write(struct.pack("<3qQ4qQ", len(V), len(T), c["n"], c["seed"], int(c["stratified"]), c["stats"][0], c["stats"][1], k, int(c["hash"], 16)))
            f.write(np.ascontiguousarray(V, f32).tobytes() + Cs.vertex_colors(V).tobytes() + np.ascontiguousarray(T, np.int32).tobytes())
            for key in ("points", "normals", "colors", "weights"):
                assert len(c[key]) == 3 * k
                f.write(_bits(c[key]).tobytes())
            f.write(np.array(c["triangles"], np.int32).tobytes())
    return len(cases)


def test_model_reproduces_the_recorded_cases():
    """tests/golden/mesh_sample_cases.json is what tests/mesh_sample_cases.py records from the model today."""
    doc = Cs.load()
    assert [(c["mesh"], c["n"], c["seed"], c["stratified"]) for c in doc["cases"]] == [(a, n, s, st) for a, _, n, s, st in Cs.RECORDED]
    assert doc["cases"] == [Cs.record(*c) for c in Cs.RECORDED]
    assert os.path.getsize(Cs.FIXTURE) < 64 << 10


def test_mesh_sample_cpp_host_layer_compiles(tmp_path):
    """CPU-side: SdfKit::MeshSdf::SamplePoints compiles and links against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_mesh_sample_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    assert _vectors(vec) == len(Cs.RECORDED)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "3 tests, 0 failures" in p.stdout
