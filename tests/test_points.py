"""CPU checks of KdTree / IterativeClosestPoint: the numpy model (tests/points_model.py) reproduces the reference's own
answers and its translation formula, and the new C-ABI entry points exist and refuse to run without a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from sdfkit_amd import _native as N
from sdfkit_amd.raymarch import Matrix4x4
from tests import points_model as PM

f32 = np.float32
ENTRY_POINTS = ["sdfk_points_create", "sdfk_points_create_device", "sdfk_points_add", "sdfk_points_add_device",
                "sdfk_points_count", "sdfk_points_search", "sdfk_points_search_device", "sdfk_points_stats",
                "sdfk_points_free", "sdfk_icp_register", "sdfk_icp_register_device"]


def test_model_three_points_kdtree():
    """KdTreeTests.ThreePoints: nearest (0, 1, 0) at 0.5."""
    idx, dist, near = PM.nearest(PM.THREE_POINTS, [[0.0, 1.5, 0.0]])
    assert idx[0] == 1 and list(near[0]) == [0, 1, 0]
    assert abs(float(dist[0]) - 0.5) <= 1e-4


def test_model_nearest_rules():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [-1, 0, 0]], f32)
    idx, dist, near = PM.nearest(pts, [[0.5, 0, 0], [0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [3e38, 0, 0]])
    assert list(idx[:2]) == [0, 0]                 # ties: the lowest index
    assert list(idx[2:4]) == [-1, -1] and dist[2] == PM.FLT_MAX and list(near[2]) == [0, 0, 0]
    assert idx[4] == -1 and dist[4] == PM.FLT_MAX  # d2 overflows to inf for every point: none counts


@pytest.mark.parametrize("name", sorted(PM.reference_transforms()))
def test_model_reference_icp_cases(name):
    """The six IterativeClosestPointTests cases at their tolerances (1e-4 translation and points, 1e-6 diagonal)."""
    pts, expected, keep = PM.reference_transforms()[name]

    def reg(static, dynamic):
        total, iters, _ = PM.register(static, dynamic)
        assert 1 <= iters < 100
        return total
    PM.check_reference_case(pts, expected, keep, reg)


def test_model_translation_is_the_references_not_kabsch():
    """The step's translation is Transform(pmean, Invert(R)) - qmean (IterativeClosestPoint.cs:176-193): with R != I it does
    not carry the filtered mean of p onto that of q, and the iterations differ from a textbook step's."""
    pts = PM.random_points_100()
    rx = Matrix4x4.CreateRotationX(f32(20.0) * PM.DEG)
    dyn = PM.transform_points(pts, rx)
    step, info = PM.icp_step(pts, dyn)
    _, inv_r = Matrix4x4.Invert(np.block([[info["R"].astype(f32), np.zeros((3, 1), f32)], [np.zeros((1, 3), f32), np.ones((1, 1), f32)]]))
    assert np.array_equal(info["translation"], Matrix4x4.Transform(info["pmean"], inv_r) - info["qmean"])
    tb_step, _ = PM.icp_step(pts, dyn, textbook=True)
    assert np.abs(step - tb_step).max() > 1e-3
    moved = PM.transform_points(dyn, step)
    kept_mean_gap = np.abs(moved.mean(axis=0) - info["qmean"]).max()
    assert kept_mean_gap > 1e-3                    # the step does not land the means on each other
    a, b = dyn.copy(), dyn.copy()
    _, n_ref, s_ref = PM.register(pts, a)
    _, n_tb, s_tb = PM.register(pts, b, textbook=True)
    assert n_ref == 5                              # pinned: this cloud, 20 degrees about X
    assert np.abs(s_ref[0] - s_tb[0]).max() > 1e-3


def test_net_random_shape():
    """System.Random(0) restatement: only its shape is checked (values cannot be verified against .NET here)."""
    r = PM.NetRandom(0)
    xs = [r.NextDouble() for _ in range(1000)]
    assert all(0.0 <= x < 1.0 for x in xs) and 0.4 < np.mean(xs) < 0.6
    assert 0 <= PM.NetRandom(0).Next(10_000) < 10_000


def test_points_entry_points_exported():
    L = N.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in N.SIGNATURES


def test_points_refuse_without_device():
    """No device (or sdfk_init not called): every compute entry point returns SDFK_ERR_NO_DEVICE.  Checked in a fresh process,
    whatever this one has initialised."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", "from tests.test_points import _refusals; _refusals(); print('refusals ok')"],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "refusals ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def _refusals():
    L = N.lib()
    pts = np.zeros((3, 3), f32)
    P = C.c_void_p(pts.ctypes.data)
    h = C.c_void_p()
    prm = N.IcpParams(100, 0.01, 1e-4, 1e-5)
    total = (C.c_float * 16)()
    it = C.c_int32()
    n = C.c_int64()
    calls = {
        "sdfk_points_create": lambda: L.sdfk_points_create(P, 3, C.byref(h)),
        "sdfk_points_create_device": lambda: L.sdfk_points_create_device(P, 3, C.byref(h)),
        "sdfk_points_add": lambda: L.sdfk_points_add(None, P, 3),
        "sdfk_points_add_device": lambda: L.sdfk_points_add_device(None, P, 3),
        "sdfk_points_search": lambda: L.sdfk_points_search(None, P, 3, None, None, None),
        "sdfk_points_search_device": lambda: L.sdfk_points_search_device(None, P, 3, None, None, None),
        "sdfk_icp_register": lambda: L.sdfk_icp_register(None, C.byref(prm), P, 3, total, C.byref(it)),
        "sdfk_icp_register_device": lambda: L.sdfk_icp_register_device(None, C.byref(prm), P, 3, total, C.byref(it)),
    }
    for name, call in calls.items():
        assert call() == N.ERR_NO_DEVICE, name
    assert not h.value
    # accessors of a set that cannot exist: argument errors
    assert L.sdfk_points_count(None, C.byref(n)) == N.ERR_INVALID
    L.sdfk_points_free(None)
