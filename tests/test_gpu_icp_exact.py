"""IterativeClosestPoint on the MI355X, bit for bit:

1. device == host build: tests/cpp/icp_solve_host.cpp compiled by hipcc with the library's flags and -DICP_SOLVE_ON_DEVICE runs the
   cases of tests/test_icp_solve.py one lane per case, as ONE child process under a time limit; R, step, total and converged are
   bit-equal to the g++ build (which the CPU file proves bit-equal to the numpy model);
2. through the ABI: for every MaxIterations = k up to the model's iteration count, total, Iterations and the moved points equal
   tests/points_model.py::register_exact -- the two clouds of tests/test_gpu_points.py, the six reference cases, and n at every
   boundary of the reduction grid (256 threads, 256 blocks, a stride of 65536);
3. the branches of the solve and of the filter, on clouds whose correspondences are known by construction (MaxIterations = 1): each
   asserts in the MODEL that the branch was reached, and that the library equals the model;
4. non-finite dynamic points: refused by the host form, unchecked (and as the contract says) in the device form."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from sdfkit_amd import build as B
from sdfkit_amd.raymarch import Matrix4x4
from tests import points_model as PM
from tests import test_icp_solve as T
from tests.test_gpu_points import _mesh_vertices

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
EPS32 = float(np.finfo(f32).eps)


# ---- 1. device against host, directly ----
def test_device_solve_equals_host_build(gpu, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "icp_solve_device")
    c = subprocess.run([hipcc] + B.CFLAGS + ["-DICP_SOLVE_ON_DEVICE", os.path.join(T.ROOT, "tests", "cpp", "icp_solve_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-4000:]
    rows, kind, names = T.all_solve_cases()
    _, scaled = T.scaling_rows()
    rows = np.concatenate([rows, T.solve_rows(scaled.reshape(-1, 3, 3))])
    host = T.runner(T.build_host(tmp_path), tmp_path)("solve", rows)
    os.makedirs(tmp_path / "dev")
    dev = T.runner(exe, tmp_path / "dev", prefix=("timeout", "-k", "10", "120"))("solve", rows)   # (asserts exit status 0: nothing else runs after a failure)
    bad = np.flatnonzero(~T.same_bits(dev, host).all(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], dev[bad[0]], host[bad[0]])


# ---- 2. through the ABI, bit for bit ----
def _check_exact(static, dynamic, max_iterations=100, good=f32(0.01)):
    """total, Iterations and the moved points of every run limited to k iterations equal the model's; -> the model's details"""
    ref = dynamic.copy()
    _, iters, totals, infos = PM.register_exact(static, ref, max_iterations, good)
    icp = K.IterativeClosestPoint(static)
    icp.GoodCorrespondenceDistance = good
    for k in range(1, iters + 1):
        icp.MaxIterations = k
        pts = dynamic.copy()
        got = icp.RegisterPoints(pts)
        assert icp.Iterations == k
        assert T.same_bits(got, totals[k - 1]).all(), (k, got, totals[k - 1])
        bad = np.flatnonzero(~T.same_bits(pts, infos[k - 1]["points"]).all(axis=1))
        assert len(bad) == 0, (k, len(bad), bad[:5], pts[bad[:5]], infos[k - 1]["points"][bad[:5]])
    if iters < max_iterations:                         # the model converged: so does the library, at the same iteration
        icp.MaxIterations = max_iterations
        assert T.same_bits(icp.RegisterPoints(dynamic.copy()), totals[-1]).all() and icp.Iterations == iters
    return infos


def test_random_cloud_exact(gpu):
    rs = np.random.default_rng(11)
    P = (rs.random((3000, 3), dtype=f32) - f32(0.5))
    xf = Matrix4x4.Multiply(Matrix4x4.CreateRotationY(f32(3.0) * PM.DEG), Matrix4x4.CreateTranslation(f32(0.02), 0, f32(-0.01)))
    assert len(_check_exact(P, PM.transform_points(P, xf))) >= 2


def test_mesh_vertices_exact(gpu):
    V = _mesh_vertices("union8", 40)
    xf = Matrix4x4.Multiply(Matrix4x4.CreateRotationX(f32(2.0) * PM.DEG), Matrix4x4.CreateTranslation(0, f32(0.05), 0))
    assert len(_check_exact(V, PM.transform_points(V, xf))) >= 2


@pytest.mark.parametrize("name", sorted(PM.reference_transforms()))
def test_reference_cases_exact(gpu, name):
    pts, expected, keep = PM.reference_transforms()[name]
    _, moved = PM.transform_for_test(pts, expected, keep)
    _check_exact(pts, moved)


def _grid_case(n):
    rs = np.random.default_rng(1000 + n)
    S = (rs.random((2000, 3), dtype=f32) - f32(0.5))
    xf = Matrix4x4.Multiply(Matrix4x4.CreateRotationY(f32(2.0) * PM.DEG), Matrix4x4.CreateTranslation(f32(0.01), f32(-0.02), 0))
    D = S[rs.integers(0, len(S), n)] + rs.normal(0, 0.002, (n, 3)).astype(f32)
    return S, PM.transform_points(D.astype(f32), xf)


# (the brute-force model costs n x 2000 distances per iteration: fewer iterations for the larger n)
@pytest.mark.parametrize("n,iters", [(1, 3), (2, 3), (255, 3), (256, 3), (257, 3), (65535, 1), (65536, 1), (65537, 2), (131073, 1)])
def test_reduction_grid_boundaries_exact(gpu, n, iters):
    S, D = _grid_case(n)
    infos = _check_exact(S, D, iters)
    assert 1 <= len(infos) <= iters and (n == 1) == infos[0]["s0_zero"]   # (one point: on its static point after one step, converged at the second)


def test_device_form_equals_host_form(gpu):
    import torch
    S, D = _grid_case(65537)
    N.bind_torch_stream()
    icp = K.IterativeClosestPoint(S)
    icp.MaxIterations = 2
    host_pts = D.copy()
    host_total = icp.RegisterPoints(host_pts)
    dev = torch.from_numpy(D.copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    dev_total = icp.RegisterDevicePoints(dev.data_ptr(), len(D))
    N.check(N.lib().sdfk_synchronize())
    assert icp.Iterations == 2 and T.same_bits(dev_total, host_total).all() and T.same_bits(dev.cpu().numpy(), host_pts).all()


# ---- 3. the branches ----
def _one_step(static, dynamic, good=f32(0.01)):
    return _check_exact(static, dynamic, 1, good)[0]


def _took(static, dynamic, index):
    """the construction's claim: dynamic point i takes static point index[i]"""
    got = PM.nearest(static, dynamic)[0]
    assert np.array_equal(got, np.asarray(index, np.int32)), np.flatnonzero(got != index)[:5]


def test_reflection(gpu):
    """A static set symmetric about the plane x = 0 (a lattice in y, z) with a small chiral perturbation (x within +-0.02); the
    dynamic set is its mirror image.  Every mirrored point takes the point it came from (spacing 0.5, offsets below 0.04), so
    C_xx < 0 < C_yy, C_zz: det C < 0, and the best ROTATION is wanted.  The model goes through detv < 0, d3 = -1.  (d3 is the sign of
    det V after the sort, U being completed to det +1, so a reflection shows as d3 = -1 or as a flipped u3 depending on the parity
    of the rotations and the sort: the seed is one where it is d3.)"""
    rs = np.random.default_rng(0)
    g = np.arange(-3, 4, dtype=f32) * f32(0.5)
    yz = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    S = np.concatenate([rs.uniform(-0.02, 0.02, (len(yz), 1)), yz], axis=1).astype(f32)
    D = (S * np.array([-1, 1, 1], f32)).astype(f32)
    _took(S, D, np.arange(len(S)))
    info = _one_step(S, D)
    assert np.linalg.det(info["C"]) < 0 and info["detv"] < 0 and info["d3"] == -1.0 and abs(np.linalg.det(info["R"]) - 1) <= 64 * T.EPS


def test_collinear_clouds(gpu):
    """points i (1, 2, 2), i = -10 .. 10, and the same shifted by (1, 2, 2) / 16 along the line: every coordinate, difference from the
    mean and product is an exact multiple of one pattern, so C = c (1, 2, 2)^T (1, 2, 2) has rank 1 exactly"""
    u = np.array([1, 2, 2], f32)
    S = (np.arange(-10, 11, dtype=f32)[:, None] * u).astype(f32)
    D = (S + u / f32(16)).astype(f32)
    _took(S, D, np.arange(21))
    info = _one_step(S, D)
    assert info["rank1"] and not info["s0_zero"] and np.array_equal(info["C"], info["C"][0, 0] * np.outer(u, u).astype(f64))
    # R is not unique but takes the line to itself, so the moved points stay on it -- within the reference's own tolerance for
    # registered points (1e-4: f32 products of coordinates up to 30 with a step matrix rounded to f32)
    moved = info["points"].astype(f64)
    off = np.linalg.norm(np.cross(moved, u.astype(f64) / 3.0), axis=1)
    assert off.max() <= 1e-4 and np.abs(moved - S).max() <= 1e-4


def test_coplanar_clouds(gpu):
    g = np.arange(-4, 5, dtype=f32)
    S = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    S = np.concatenate([S, np.zeros((len(S), 1), f32)], axis=1).astype(f32)
    D = PM.transform_points(S, Matrix4x4.CreateTranslation(f32(0.03), f32(-0.02), 0))
    D[:, :2] += (np.random.default_rng(5).normal(0, 0.01, (len(S), 2))).astype(f32)
    _took(S, D, np.arange(len(S)))
    info = _one_step(S, D)
    assert not info["rank1"] and (info["C"][2] == 0).all() and (info["C"][:, 2] == 0).all() and np.linalg.matrix_rank(info["C"]) == 2
    assert (info["points"][:, 2] == 0).all()


@pytest.mark.parametrize("n", [1, 300])
def test_one_point_and_identical_points(gpu, n):
    """C = 0: R = I, and the step is the pure translation onto the nearest static point"""
    rs = np.random.default_rng(6)
    S = rs.uniform(-2, 2, (50, 3)).astype(f32)
    D = np.tile((S[17] + np.array([0.01, -0.02, 0.015], f32)).astype(f32), (n, 1))
    _took(S, D, np.full(n, 17))
    info = _one_step(S, D)
    assert info["s0_zero"] and np.array_equal(info["R"], np.eye(3)) and (info["C"] == 0).all()
    # q - p, its negation through Invert, p + it: three roundings of coordinates below 4
    assert np.abs(info["points"].astype(f64) - S[17]).max() <= 3 * EPS32 * 4


def test_lattice_of_equal_distances(gpu):
    """every point 0.004 from its lattice point along x: the distances differ by the rounding of x + 0.004 at most, sd is 0 or a
    rounding, and dist <= (float)mean (+ 3 sd) decides who is kept: the library's result is the model's, whose count is stated"""
    g = np.arange(0, 7, dtype=f32)
    S = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    D = (S + np.array([0.004, 0, 0], f32)).astype(f32)
    _took(S, D, np.arange(len(S)))
    info = _one_step(S, D)
    d = PM.nearest(S, D)[1]
    assert info["bracket"] == 0 and len(np.unique(d)) > 1 and float(info["sd"]) < 1e-6
    assert info["kept"] == int((d <= info["dist_max"]).sum()) and 0 < info["kept"] <= len(S)
    print("lattice: kept", info["kept"], "of", len(S), "distMax", info["dist_max"], "distinct distances", len(np.unique(d)))


@pytest.mark.parametrize("bracket,offset", [(0, 0.005), (1, 0.02), (2, 0.045), (3, 0.09)])
def test_every_dist_max_bracket(gpu, bracket, offset):
    """a lattice of spacing 1 and points `offset` (+- 30 %) from it, GoodCorrespondenceDistance = 0.01: the mean distance falls in
    bracket 0 (< good), 1 (< 3 good), 2 (< 6 good), 3 (the rest); five points four times as far"""
    rs = np.random.default_rng(20 + bracket)
    g = np.arange(-3, 4, dtype=f32)
    S = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    dirs = rs.standard_normal(S.shape)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    far = rs.uniform(0.7, 1.3, (len(S), 1))
    far[::70] = 4.0                                    # five outliers (0.36 at most: still their lattice point's)
    D = (S + dirs * (offset * far)).astype(f32)
    _took(S, D, np.arange(len(S)))
    info = _one_step(S, D)
    # the last bracket's distMax is above 0.5, so it keeps everything here; the others drop at least the outliers
    assert info["bracket"] == bracket and (info["kept"] == len(S) if bracket == 3 else 0 < info["kept"] <= len(S) - 5)


def test_thirty_degree_rotation(gpu):
    """the six unit axis points as the static set; dynamic points at radius 5 to 50 within 10 degrees of an axis, turned by 30
    degrees about z: each stays inside the Voronoi cone of its axis point (45 degrees), so the correspondences are the construction's"""
    rs = np.random.default_rng(8)
    S = np.concatenate([np.eye(3), -np.eye(3)]).astype(f32)
    axis = rs.integers(0, 6, 400)
    jitter = rs.uniform(-1, 1, (400, 3)) * np.tan(np.radians(10)) / np.sqrt(2)
    P = (S[axis] + jitter * (S[axis] == 0)) * rs.uniform(5, 50, (400, 1))
    c, s = np.cos(np.radians(30)), np.sin(np.radians(30))
    D = (P @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])).astype(f32)
    _took(S, D, axis)
    info = _one_step(S, D)
    assert info["bracket"] == 3 and info["rotations"] >= 3 and abs(np.linalg.det(info["R"]) - 1) <= 64 * T.EPS


# ---- 4. non-finite dynamic points ----
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_host_form_refuses_nonfinite_points(gpu, bad):
    S, D = _grid_case(300)
    D[123, 1] = bad
    before = D.copy()
    tree = K.KdTree(S)
    total = (C.c_float * 16)(*([7.0] * 16))
    iters = C.c_int32(-5)
    prm = N.IcpParams(3, 0.01, 1e-4, 1e-5)
    r = N.lib().sdfk_icp_register(tree.handle, C.byref(prm), C.c_void_p(D.ctypes.data), len(D), total, C.byref(iters))
    assert r == N.ERR_INVALID and iters.value == -5 and list(total) == [7.0] * 16
    assert T.same_bits(D, before).all()
    with pytest.raises(N.SdfKitNativeError) as e:
        K.IterativeClosestPoint(S).RegisterPoints(D)
    assert e.value.status == N.ERR_INVALID and T.same_bits(D, before).all()


@pytest.mark.parametrize("n", [1, 300])
def test_device_form_takes_nonfinite_points_as_the_contract_says(gpu, n):
    """unchecked: the point's correspondence is (first static point, FLT_MAX), which is what the model's search returns as well"""
    import torch
    S, D = _grid_case(n)
    D[n // 2, 0] = np.nan
    idx, dist, cor = PM.nearest(S, D[n // 2:n // 2 + 1])
    assert idx[0] == -1 and dist[0] == PM.FLT_MAX and np.array_equal(cor[0], S[0])
    ref = D.copy()
    total, iters, _, infos = PM.register_exact(S, ref, 2)
    assert np.isnan(total).any() == (n == 1) and (n == 1 or infos[0]["kept"] < n)   # n = 1: the whole transform is NaN; else filtered out
    N.bind_torch_stream()
    dev = torch.from_numpy(D.copy()).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    icp = K.IterativeClosestPoint(S)
    icp.MaxIterations = 2
    got = icp.RegisterDevicePoints(dev.data_ptr(), n)
    N.check(N.lib().sdfk_synchronize())
    assert icp.Iterations == iters and T.same_bits(got, total).all() and T.same_bits(dev.cpu().numpy(), ref).all()
