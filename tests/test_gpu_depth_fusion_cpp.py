"""Builds and runs tests/cpp/depth_fusion_suite.cpp: SdfKit::DepthFusion (Integrate, ToVoxels, Weights, the stats) and
SdfKit::DepthToPoints (include/SdfKit.hpp) over a few of the cases of tests/depth_fusion_cases.py, against vectors written here with
the numpy model (tests/depth_fusion_model.py), bit for bit.  On the CPU: the layer compiles and links."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import depth_fusion_cases as Cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32, i64, u32 = np.float32, np.int32, np.int64, np.uint32
VOLUMES = ("sphere_5x6x7_carve", "sphere_2x3x261_open", "image_2x2_alternating", "camera_inside", "exact_axis", "odd_depths_carve",
           "sequence_max_weight", "sequence_weight_half")
FRAMES = ("2x2_none", "3x5_alternating", "16x16_all", "64x48_alternating", "257x1_all", "scene_64x48", "scene_no_rgb")


def _build(tmp):
    from sdfkit_amd import _native as N
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "depth_fusion_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "depth_fusion_suite.cpp"), "-o", exe,
           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def _vectors(path):
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(VOLUMES)))
        for name in VOLUMES:
            c = Cs.volume_case(name)
            D, W, stats = Cs.volume_model(name)
            assert c["z0"] == 0 and not c["W0"].any() and np.all(c["D0"] == c["D0"].flat[0])   # what the class starts from
            f.write(struct.pack("<5q9f", *c["shape"], len(c["frames"]), int(bool(c["frames"][0]["flags"])), c["truncation"], c["D0"].flat[0],
                                c["max_weight"], *c["mn"], *c["mx"]))
            for fr, st in zip(c["frames"], stats):
                assert set(fr["lens"]) <= {"nearPlaneDistance"}
                h, w = fr["depth"].shape
                pos, target, up = fr["cam"]
                f.write(struct.pack("<2q13f", w, h, fr["weight"], fr["depth_min"], fr["depth_max"], fr["lens"].get("nearPlaneDistance", 1.0),
                                    *pos, *target, *up))
                f.write(fr["depth"].tobytes() + np.asarray(st, i64).tobytes())
            f.write(np.ascontiguousarray(D).view(u32).tobytes() + np.ascontiguousarray(W).view(u32).tobytes())
        f.write(struct.pack("<q", len(FRAMES)))
        for name in FRAMES:
            c = Cs.frame_case(name)
            pts, cols, pix = Cs.frame_model(name)
            pos, target, up = c["cam"]
            f.write(struct.pack("<4q9f", c["width"], c["height"], int(c["rgb"] is not None), len(pix), *pos, *target, *up))
            f.write(c["depth"].tobytes() + (b"" if c["rgb"] is None else c["rgb"].tobytes()))
            f.write(np.ascontiguousarray(pts).view(u32).tobytes() + (b"" if cols is None else np.ascontiguousarray(cols).view(u32).tobytes()) +
                    pix.astype(i32).tobytes())
    return len(VOLUMES) + len(FRAMES)


def test_depth_fusion_cpp_host_layer_compiles(tmp_path):
    """CPU-side: the members compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_depth_fusion_suite_through_cpp_host_layer(tmp_path, gpu):
    exe = _build(str(tmp_path))
    vec = str(tmp_path / "vectors.bin")
    n = _vectors(vec)
    p = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert f"{n} tests, 0 failures" in p.stdout
