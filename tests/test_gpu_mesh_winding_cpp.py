"""Builds and runs tests/cpp/mesh_winding_suite.cpp: WindingNumber, Contains, ToVoxels / SampleInto with a MeshSign of SdfKit::MeshSdf
and WindingNumber, Contains of SdfKit::Mesh (include/SdfKit.hpp) over a few of the cases of tests/mesh_winding_cases.py, against
vectors written here with the numpy models (tests/mesh_winding_model.py; the distances: tests/meshsdf_model.py), bit for bit.  On the
CPU: the layer compiles and links."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_winding_cases as Cs
from tests import meshsdf_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32, u32 = np.float32, np.int32, np.uint32
POINTS = ("cube", "octahedron_inside_out", "cube_no_lid", "two_cubes", "degenerate", "hemisphere", "bad_queries", "count_257")
VOLUMES = ("two_cubes", "cube_no_lid", "banded_cube")


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "mesh_winding_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "mesh_winding_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _vectors(path):
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(POINTS)))
        for name in POINTS:
            c, want = Cs.case(name), Cs.model(name)
            f.write(struct.pack("<3q", len(c["V"]), len(c["T"]), len(c["Q"])))
            f.write(c["V"].tobytes() + c["T"].tobytes() + c["Q"].tobytes())
            f.write(want.winding.view(u32).tobytes() + want.inside.astype(np.uint8).tobytes())
        f.write(struct.pack("<q", len(VOLUMES)))
        for name in VOLUMES:
            c = Cs.case(name)
            assert c["z0"] == 0 and c["nz"] == c["n"][2]
            parity, _ = MM.volume(c["V"], c["T"].reshape(-1), c["mn"], c["mx"], c["n"], band=c["band"])
            inside = Cs.volume_model(name).inside.reshape(parity.shape)
            winding = np.where(inside, -np.abs(parity), np.abs(parity)).astype(f32)
            f.write(struct.pack("<5q7f", len(c["V"]), len(c["T"]), *c["n"], *c["mn"], *c["mx"], c["band"]))
            f.write(c["V"].tobytes() + c["T"].tobytes())
            f.write(np.ascontiguousarray(parity, f32).view(u32).tobytes() + np.ascontiguousarray(winding).view(u32).tobytes())
    return len(POINTS) + len(VOLUMES)


def test_mesh_winding_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the members compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_mesh_winding_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    n = _vectors(vec)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert f"{n} tests, 0 failures" in p.stdout
