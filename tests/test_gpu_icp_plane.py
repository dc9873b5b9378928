"""Point-to-plane IterativeClosestPoint on the MI355X (sdfk_icp_register_plane[_device]), bit for bit against
tests/icp_plane_model.py::register_plane_exact: total, the moved points, the iteration count and the stats.

1. the height-field case (a 48 x 48 grid of z = 0.25 sin(3x) cos(2y) + 0.1 x y with analytic normals; off-grid surface points,
   rotated and moved) at dynamic sizes 1, 255, 256, 257, 700 and 65 536 + 3 -- the last puts a second element on a reduction thread;
2. the host form and the device form are equal;
3. a static set with some zero normals: those correspondences are dropped, stats[0] is the model's;
4. the plane case: rows and columns 2, 3, 4 of A are exactly zero, 3 eigenvalues are retained;
5. max_iterations = 0: the identity, untouched points, zero stats; every refusal leaves points and outputs untouched;
6. the Python layer's metric and StaticNormals rules;
7. the worth of it: the device reproduces the iteration counts recorded from the two models in tests/golden/icp_plane_cases.json,
   and the plane metric needs fewer iterations and ends nearer the true positions."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from tests import icp_plane_model as M
from tests import points_model as PM
from tests.test_icp_plane_solve import GOLDEN
from tests.test_icp_solve import same_bits

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def _static():
    return M.height_field_static()


@functools.lru_cache(maxsize=None)
def _model(n, max_iterations):
    """the model's registration of the height-field case with n dynamic points -> (dynamic, total, iterations, totals, infos)"""
    S, Nn = _static()
    D0, D = M.height_field_dynamic(n)
    total, iters, totals, infos = M.register_plane_exact(S, Nn, D.copy(), max_iterations)
    return D, total, iters, totals, infos


def _icp(S, Nn, max_iterations=100):
    icp = K.IterativeClosestPoint(S)
    icp.StaticNormals = Nn
    icp.MaxIterations = max_iterations
    return icp


def _equal(icp, pts, got, total, info, iters):
    assert icp.Iterations == iters
    assert same_bits(got, total).all(), (got, total)
    bad = np.flatnonzero(~same_bits(pts, info["points"]).all(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], pts[bad[:5]], info["points"][bad[:5]])
    assert icp.LastStats["raw"] == [int(v) for v in info["stats"]], (icp.LastStats, info["stats"])


# ---- 1. the height-field case at every boundary of the reduction grid ----
# (the brute-force model costs n x 2304 distances per iteration: one iteration for the largest n)
@pytest.mark.parametrize("n,max_iterations", [(1, 100), (255, 100), (256, 100), (257, 100), (700, 100), (65536 + 3, 1)])
def test_height_field_exact(gpu, n, max_iterations):
    S, Nn = _static()
    D, total, iters, totals, infos = _model(n, max_iterations)
    assert 1 <= iters <= max_iterations and (iters < 10 or n == 1)
    icp = _icp(S, Nn)
    for k in range(1, iters + 1) if n <= 700 else [iters]:
        icp.MaxIterations = k
        pts = D.copy()
        _equal(icp, pts, icp.RegisterPoints(pts), totals[k - 1], infos[k - 1], k)
    if iters < max_iterations:                         # the model converged: so does the library, at the same iteration
        icp.MaxIterations = max_iterations
        pts = D.copy()
        _equal(icp, pts, icp.RegisterPoints(pts), total, infos[-1], iters)
        assert icp.LastStats["converged"] and icp.LastStats["retained"] == infos[-1]["retained"]


# ---- 2. the two forms ----
def test_device_form_equals_host_form(gpu):
    import torch
    S, Nn = _static()
    D, total, iters, totals, infos = _model(700, 100)
    N.bind_torch_stream()
    icp = _icp(S, Nn)
    dev = torch.from_numpy(D.copy()).to(torch.device("cuda:0"))
    nrm = torch.from_numpy(Nn.copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    got = icp.RegisterDevicePoints(dev.data_ptr(), len(D), normals_dev=nrm.data_ptr())
    N.check(N.lib().sdfk_synchronize())
    _equal(icp, dev.cpu().numpy(), got, total, infos[-1], iters)
    dev = torch.from_numpy(D.copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    got = icp.RegisterDevicePoints(dev.data_ptr(), len(D))       # (the wrapper uploads StaticNormals)
    N.check(N.lib().sdfk_synchronize())
    _equal(icp, dev.cpu().numpy(), got, total, infos[-1], iters)


# ---- 3. zero normals ----
def test_zero_normals_are_dropped(gpu):
    S, Nn = _static()
    Nn = Nn.copy()
    Nn[::5] = 0
    Nn[2::10] = f32(-0.0)
    _, D = M.height_field_dynamic(700)
    ref = D.copy()
    total, iters, totals, infos = M.register_plane_exact(S, Nn, ref, 3)
    dropped = [int((PM.nearest(S, D)[1] <= i["dist_max"]).sum()) - i["kept"] for i in infos[:1]]
    assert dropped[0] > 50 and 0 < infos[0]["kept"] < 700 - 50
    icp = _icp(S, Nn, 3)
    pts = D.copy()
    _equal(icp, pts, icp.RegisterPoints(pts), total, infos[-1], iters)
    assert icp.LastStats["kept"] == infos[-1]["kept"]


# ---- 4. the plane ----
def test_plane_case_retains_three(gpu):
    S, Nn, D = M.plane_case()
    ref = D.copy()
    total, iters, totals, infos = M.register_plane_exact(S, Nn, ref)
    assert all(i["retained"] == 3 for i in infos)
    icp = _icp(S, Nn)
    for k in range(1, iters + 1):
        icp.MaxIterations = k
        pts = D.copy()
        _equal(icp, pts, icp.RegisterPoints(pts), totals[k - 1], infos[k - 1], k)
        assert icp.LastStats["raw"][3] == 3


# ---- 5. no iteration, and the refusals ----
def test_no_iterations_is_the_identity(gpu):
    S, Nn = _static()
    _, D = M.height_field_dynamic(300)
    icp = _icp(S, Nn, 0)
    pts = D.copy()
    got = icp.RegisterPoints(pts)
    assert np.array_equal(got, np.eye(4, dtype=f32)) and same_bits(pts, D).all() and icp.Iterations == 0
    assert icp.LastStats["raw"] == [0, 0, 0, 0]


def _raw_call(tree, prm, normals, pts, n, device=False):
    total = (C.c_float * 16)(*([7.0] * 16))
    iters = C.c_int32(-5)
    stats = (C.c_int64 * 4)(-9, -9, -9, -9)
    fn = N.lib().sdfk_icp_register_plane_device if device else N.lib().sdfk_icp_register_plane
    r = fn(tree.handle, C.byref(prm), normals, pts, n, total, C.byref(iters), stats)
    return r, list(total) == [7.0] * 16 and iters.value == -5 and list(stats) == [-9] * 4


@pytest.mark.parametrize("what", ["null_normals", "no_points", "negative_iterations", "nan_point", "inf_point", "nan_normal", "inf_normal"])
def test_refusals_touch_nothing(gpu, what):
    S, Nn = _static()
    Nn = Nn.copy()
    _, D = M.height_field_dynamic(300)
    prm = N.IcpParams(3, 0.01, 1e-4, 1e-5)
    n = len(D)
    if what == "negative_iterations":
        prm = N.IcpParams(-1, 0.01, 1e-4, 1e-5)
    if what == "no_points":
        n = 0
    if what.endswith("_point"):
        D[123, 1] = np.nan if what.startswith("nan") else -np.inf
    if what.endswith("_normal"):
        Nn[len(Nn) - 1, 2] = np.nan if what.startswith("nan") else np.inf
    before = D.copy()
    tree = K.KdTree(S)
    normals = C.c_void_p() if what == "null_normals" else C.c_void_p(Nn.ctypes.data)
    r, untouched = _raw_call(tree, prm, normals, C.c_void_p(D.ctypes.data), n)
    assert r == N.ERR_INVALID and untouched and same_bits(D, before).all()
    if what in ("null_normals", "no_points", "negative_iterations"):       # the device form checks these too (no device memory is read)
        r, untouched = _raw_call(tree, prm, normals, C.c_void_p(D.ctypes.data), n, device=True)
        assert r == N.ERR_INVALID and untouched


# ---- 6. the Python layer ----
def test_metric_and_static_normals_rules(gpu):
    S, Nn = _static()
    _, D = M.height_field_dynamic(300)
    icp = K.IterativeClosestPoint(S)
    icp.MaxIterations = 2
    assert icp.StaticNormals is None and icp.LastStats is None
    with pytest.raises(ValueError):
        icp.RegisterPoints(D.copy(), metric="plane")              # no normals
    with pytest.raises(ValueError):
        icp.RegisterPoints(D.copy(), metric="planar")
    with pytest.raises(ValueError):
        icp.StaticNormals = Nn[:-1]
    with pytest.raises(ValueError):
        icp.StaticNormals = Nn.reshape(-1)
    with pytest.raises(ValueError):
        icp.AddStaticPoints(S[:4], normals=Nn[:4])                # normals for the new points only
    point_total = icp.RegisterPoints(D.copy())                    # None without normals: point to point
    assert icp.LastStats is None
    icp.StaticNormals = Nn.astype(f64)                            # (converted to float32)
    assert icp.StaticNormals.dtype == f32 and icp.StaticNormals.shape == (len(S), 3)
    plane_total = icp.RegisterPoints(D.copy())                    # None with normals: point to plane
    assert icp.LastStats is not None and not same_bits(plane_total, point_total).all()
    assert same_bits(icp.RegisterPoints(D.copy(), metric="plane"), plane_total).all()
    assert same_bits(icp.RegisterPoints(D.copy(), metric="point"), point_total).all() and icp.LastStats is None
    with pytest.raises(ValueError):
        icp.AddStaticPoints(S[:4])                                # would leave the normals short
    with pytest.raises(ValueError):
        icp.AddStaticPoints(S[:4], normals=Nn[:3])
    assert icp.StaticTree.TotalPoints == len(S)                   # nothing was added by the refused calls
    icp.AddStaticPoints(S[:4] + f32(5.0), normals=Nn[:4])
    assert icp.StaticTree.TotalPoints == len(S) + 4 and icp.StaticNormals.shape == (len(S) + 4, 3)
    assert same_bits(icp.RegisterPoints(D.copy()), plane_total).all()   # (the far points are nobody's nearest)
    icp.StaticNormals = None
    assert same_bits(icp.RegisterPoints(D.copy()), point_total).all()
    # GlobalRegisterPoints stays point to point
    a = K.IterativeClosestPoint(S).GlobalRegisterPoints([S], [D.copy()])
    icp2 = K.IterativeClosestPoint(S)
    assert same_bits(a[0], icp2.RegisterPoints(D.copy())).all()


# ---- 7. it is worth having ----
def test_plane_metric_beats_point_metric(gpu):
    with open(GOLDEN) as f:
        rec = json.load(f)
    S, Nn = _static()
    D0, D = M.height_field_dynamic(700)
    icp = K.IterativeClosestPoint(S)
    pts = D.copy()
    icp.RegisterPoints(pts)
    it_point, rms_point = icp.Iterations, M.rms(pts, D0)
    icp.StaticNormals = Nn
    pts = D.copy()
    icp.RegisterPoints(pts)
    it_plane, rms_plane = icp.Iterations, M.rms(pts, D0)
    print("point:", it_point, rms_point, "plane:", it_plane, rms_plane)
    assert it_point == rec["point"]["iterations"] and it_plane == rec["plane"]["iterations"]
    assert it_plane < it_point and rms_plane < rms_point
