"""Builds and runs tests/cpp/raymarch_suite.cpp: SdfKit::RayMarcher of the C++ host layer include/SdfKit.hpp -- its Matrix4x4
arithmetic, its camera derivation and its call of sdfk_raymarch -- against the oracle's depth and colour images, every float as bits.
The vectors are written here at run time from the oracle (they depend on the host's tanf, which the oracle and the header share on
whichever machine runs them): three cameras x two lenses x two shapes x two iteration counts for each of four scenes the suite builds
in C++.  On the CPU: the suite compiles and links, and the oracle's images of its cases are not empty."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import raymarch_cases as R
from tests import scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CAMERAS = ["oblique", "up_z", "inside"]
LENSES = [(60.0, 1.0, 100.0), (45.0, 0.5, 250.0)]
SIZES = [(33, 21), (86, 3)]
ITERATIONS = [0, 40]


def _union_of_three():
    s = O.Scene()
    s.root = s.f_union(s.f_translate(s.f_sphere(0.6), -1, 0, 0), s.f_union(s.f_translate(s.f_box(0.5), 1, 0, 0), s.f_cylinder(0.4, 0.6)))
    return s


def _sphere():
    s = O.Scene(); s.sphere_w(1.0)
    return s


def _box():
    s = O.Scene(); s.box_w(1.0)
    return s


# in the order of the suite's scene numbers
SCENES = [_sphere, _box, lambda: S.readme_repeat_xy()[0], _union_of_three]


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "raymarch_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "raymarch_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _cases():
    """(scene number, camera, lens, size, iterations, oracle depth, oracle rgb) of every case"""
    for k, build in enumerate(SCENES):
        scene = build()
        for cam in CAMERAS:
            for lens in LENSES:
                for size in SIZES:
                    for iterations in ITERATIONS:
                        yield (k, cam, lens, size, iterations, *R.render(scene, cam, lens, size, iterations))


def _vectors(path):
    cases = list(_cases())
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for k, cam, lens, (w, h), iterations, depth, rgb in cases:
            pos, tgt, up = R.CAMERAS[cam]
            f.write(struct.pack("<4i", k, w, h, iterations))
            f.write(np.array([*pos, *tgt, *up, *lens], f32).tobytes())
            f.write(np.ascontiguousarray(depth, f32).tobytes() + np.ascontiguousarray(rgb, f32).tobytes())
    return len(cases)


def test_the_suites_cases_show_their_scenes():
    """every scene is hit from the outside cameras at 40 steps, in both shapes; at 0 steps the depth is the near start"""
    n = 0
    for k, cam, lens, size, iterations, depth, rgb in _cases():
        n += 1
        nan, sky, hit, nan_rgb = R.census(depth, rgb, lens[2])
        assert nan == 0 and nan_rgb == 0, (k, cam, lens, size, iterations)
        if iterations == 0:
            assert np.array_equal(depth, np.full(depth.shape, f32(lens[1]) - f32(0.1), f32))
        elif cam != "inside":
            assert hit >= (20 if size == (33, 21) else 1), (k, cam, lens, size, hit)      # (86 x 3 has one row through the scene)
        else:      # (from inside a body the march goes backwards, or through the scene into the sky)
            assert (depth != f32(lens[1]) - f32(0.1)).all(), (k, cam, lens, size)
    assert n == 4 * 24


def test_raymarch_cpp_host_layer_compiles(tmp_path):
    """CPU-side: SdfKit::RayMarcher and the suite compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_raymarch_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    assert _vectors(vec) == 4 * 24
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "4 tests, 0 failures" in p.stdout
