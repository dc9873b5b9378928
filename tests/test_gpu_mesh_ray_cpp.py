"""Builds and runs tests/cpp/mesh_ray_suite.cpp: RayCast, Occluded, Render, RenderDepth, RenderTriangles of SdfKit::MeshSdf and
RayCast, Occluded, ToImage of SdfKit::Mesh (include/SdfKit.hpp) over a few of the cases of tests/mesh_ray_cases.py, against vectors
written here with the numpy model (tests/mesh_ray_model.py), bit for bit.  On the CPU: the layer compiles and links."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_ray_cases as Cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32, u32 = np.float32, np.int32, np.uint32
CASTS = ("single_triangle", "shared_edge", "cube", "early_exit_trap", "bad_rays", "range_behind", "count_0", "count_257")
RENDERS = ("cube_2x2", "cube_colors_64x48", "sphere_colors_257x3", "inside_sphere", "near_past_front")


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "mesh_ray_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "mesh_ray_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _mesh(c):
    cols = c["colors"]
    return c["V"].tobytes() + c["T"].tobytes() + (b"" if cols is None else cols.tobytes())


def _vectors(path):
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(CASTS)))
        for name in CASTS:
            c, want = Cs.case(name), Cs.model(name)
            f.write(struct.pack("<4q2f", len(c["V"]), len(c["T"]), int(c["colors"] is not None), len(c["O"]), c["tmin"], c["tmax"]))
            f.write(_mesh(c) + c["O"].tobytes() + c["D"].tobytes())
            f.write(want.triangle.astype(i32).tobytes() + want.distance.view(u32).tobytes() + np.ascontiguousarray(want.weights).view(u32).tobytes())
        f.write(struct.pack("<q", len(RENDERS)))
        for name in RENDERS:
            c = Cs.render_case(name)
            depth, rgb, tri = Cs.render_model(name)
            pos, target, up = c["camera"]
            f.write(struct.pack("<5q11f", len(c["V"]), len(c["T"]), int(c["colors"] is not None), c["width"], c["height"], c["near"], c["far"],
                                *pos, *target, *up))
            f.write(_mesh(c))
            f.write(np.ascontiguousarray(depth).view(u32).tobytes() + np.ascontiguousarray(rgb).view(u32).tobytes() + np.ascontiguousarray(tri, i32).tobytes())
    return len(CASTS) + len(RENDERS)


def test_mesh_ray_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the members compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_mesh_ray_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    n = _vectors(vec)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert f"{n} tests, 0 failures" in p.stdout
