"""KdTree / IterativeClosestPoint on the MI355X against the numpy model (tests/points_model.py): the reference's own tests
through the Python mirror, exact search (indices equal, ties included; distances bit-equal) on clouds of every awkward
shape, and ICP step by step."""
import ctypes as C
import time

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from sdfkit_amd.raymarch import Matrix4x4
from tests import points_model as PM
from tests import scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32


def _exact(tree, static, queries):
    idx, dist, near = tree.SearchMany(queries)
    ri, rd, rn = PM.nearest(static, queries)
    bad = np.nonzero(idx != ri)[0]
    assert len(bad) == 0, (len(bad), bad[:5], idx[bad[:5]], ri[bad[:5]])
    assert np.array_equal(dist.view(np.uint32), rd.view(np.uint32))
    assert np.array_equal(near.view(np.uint32), rn.view(np.uint32))
    return idx, dist


def _mesh_vertices(name, n=48):
    _, sdf = S.CATALOGUE[name]()
    m = sdf.ToMesh([-2.5] * 3, [2.5] * 3, n, n, n, clipToBounds=False)
    return np.ascontiguousarray(np.asarray(m.Vertices, f32).reshape(-1, 3))


# ---- the reference's tests (Tests/KdTreeTests.cs, Tests/IterativeClosestPointTests.cs) ----
def test_reference_kdtree_three_points(gpu):
    tree = K.KdTree(PM.THREE_POINTS)
    assert tree.SplitAxis == 0 and tree.TotalPoints == 3
    nearest, distance = tree.Search(np.array([0.0, 1.5, 0.0], f32))
    assert list(nearest) == [0, 1, 0]
    assert abs(float(distance) - 0.5) <= 1e-4


def test_reference_kdtree_random_points(gpu):
    rng = PM.NetRandom(0)
    pts = np.array([[f32(rng.NextDouble() * 2 - 1), f32(rng.NextDouble() * 2 - 1), f32(rng.NextDouble() * 2 - 1)]
                    for _ in range(10_000)], f32) * f32(1000.0)
    tree = K.KdTree(pts)
    assert tree.TotalPoints == len(pts)
    qi = rng.Next(len(pts))
    offset = np.array([0.01, 0.01, 0.01], f32)
    nearest, distance = tree.Search(pts[qi] + offset)
    assert np.array_equal(nearest, pts[qi])
    assert abs(float(distance) - float(np.sqrt(np.float32(3) * f32(0.01) ** 2))) <= 1e-4


@pytest.mark.parametrize("name", sorted(PM.reference_transforms()))
def test_reference_icp(gpu, name):
    pts, expected, keep = PM.reference_transforms()[name]

    def reg(static, dynamic):
        return K.IterativeClosestPoint(static).RegisterPoints(dynamic)
    PM.check_reference_case(pts, expected, keep, reg)


# ---- exact search ----
def test_uniform_cube_full_brute_force(gpu):
    rs = np.random.default_rng(1)
    P = rs.random((20_000, 3), dtype=f32)
    Q = rs.random((20_000, 3), dtype=f32)
    _exact(K.KdTree(P), P, Q)


def test_million_points_sampled(gpu):
    rs = np.random.default_rng(2)
    P = (rs.random((1_000_000, 3), dtype=f32) * f32(2) - f32(1))
    Q = (rs.random((200_000, 3), dtype=f32) * f32(2.2) - f32(1.1))
    tree = K.KdTree(P)
    idx, dist, near = tree.SearchMany(Q)
    pick = rs.choice(len(Q), 2000, replace=False)
    ri, rd, rn = PM.nearest(P, Q[pick])
    assert np.array_equal(idx[pick], ri)
    assert np.array_equal(dist[pick].view(np.uint32), rd.view(np.uint32))
    assert np.array_equal(near[pick], rn)


@pytest.mark.parametrize("name", ["union8", "colored_spheres"])
def test_mesh_vertices(gpu, name):
    V = _mesh_vertices(name)
    rs = np.random.default_rng(3)
    Q = np.concatenate([V[rs.choice(len(V), 3000)] + rs.normal(0, 0.05, (3000, 3)).astype(f32),
                        rs.uniform(-2.6, 2.6, (3000, 3)).astype(f32)]).astype(f32)
    _exact(K.KdTree(V), V, Q)


def test_lattice_cell_centres_mass_ties(gpu):
    g = np.arange(12, dtype=f32)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    P = P[np.random.default_rng(4).permutation(len(P))]
    Q = (np.stack(np.meshgrid(g[:-1], g[:-1], g[:-1], indexing="ij"), -1).reshape(-1, 3) + f32(0.5)).astype(f32)
    idx, _ = _exact(K.KdTree(P), P, Q)
    assert len(np.unique(idx)) < len(idx)   # (8 equidistant points per query: the lowest index wins)


def test_duplicates(gpu):
    P = np.tile(np.array([[0.25, -1.0, 3.0]], f32), (1000, 1))
    Q = np.random.default_rng(5).normal(0, 2, (500, 3)).astype(f32)
    idx, _ = _exact(K.KdTree(P), P, Q)
    assert (idx == 0).all()
    P2 = np.concatenate([np.tile([[0, 0, 0]], (300, 1)), np.tile([[1, 0, 0]], (300, 1))]).astype(f32)
    P2 = P2[np.random.default_rng(6).permutation(600)]
    _exact(K.KdTree(P2), P2, np.concatenate([Q, [[0.5, 0, 0]]]).astype(f32))


def test_degenerate_boxes(gpu):
    rs = np.random.default_rng(7)
    line = np.zeros((5000, 3), f32)
    line[:, 1] = rs.random(5000, dtype=f32)
    plane = np.zeros((5000, 3), f32)
    plane[:, 0], plane[:, 2] = rs.random(5000, dtype=f32), rs.random(5000, dtype=f32)
    for P in (line, plane):
        Q = rs.normal(0.5, 0.7, (3000, 3)).astype(f32)
        _exact(K.KdTree(P), P, Q)


def test_collinear_cloud_beyond_2_24_points(gpu):
    """A line of more than 2^24 points: its grid is capped at 2^24 cells along the line (points_grid.h), the point at the far
    end keeps its cell, and the search stays exact."""
    rs = np.random.default_rng(13)
    n = (1 << 24) + 3_000_000
    P = np.zeros((n, 3), f32)
    P[:, 0] = rs.random(n, dtype=f32)
    P[rs.choice(n, 2, replace=False), 0] = [0.0, 1.0]   # the box's ends are points
    tree = K.KdTree(P)
    assert tree.TotalPoints == n
    grid = tree.stats()["grid"]
    assert grid[0] <= 1 << 24 and grid[1] == grid[2] == 1
    Q = np.zeros((48, 3), f32)
    Q[:, 0] = rs.random(48, dtype=f32)
    Q[:8, 0] = [1.0, 0.0, np.nextafter(f32(1), f32(2)), 1.5, -0.5, 0.5, 0.25, 0.75]
    Q[40:, 1] = rs.normal(0, 0.1, 8).astype(f32)
    _exact(tree, P, Q)


def test_far_equal_and_nonfinite_queries(gpu):
    rs = np.random.default_rng(8)
    P = rs.random((20_000, 3), dtype=f32)
    tree = K.KdTree(P)
    far = (rs.normal(0, 1, (500, 3)) * 1e4).astype(f32)
    same = P[rs.choice(len(P), 500)]
    _exact(tree, P, np.concatenate([far, same]).astype(f32))
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 3e38, 3e38]], f32)
    idx, dist, near = tree.SearchMany(bad)
    assert (idx == -1).all() and (dist == PM.FLT_MAX).all() and (near == P[0]).all()
    nearest, d = tree.Search(bad[0])
    assert np.array_equal(nearest, P[0]) and d == PM.FLT_MAX   # nearest = Point


def test_outlier_cloud_known_weak_case(gpu):
    rs = np.random.default_rng(9)
    P = np.concatenate([rs.random((100_000, 3), dtype=f32), [[1e6, 1e6, 1e6]]]).astype(f32)
    Q = rs.random((2000, 3), dtype=f32)
    tree = K.KdTree(P)
    t0 = time.perf_counter()
    tree.SearchMany(Q)
    print(f"outlier cloud: 2000 queries against 100001 points in {1e3 * (time.perf_counter() - t0):.2f} ms, grid {tree.stats()['grid']}")
    _exact(tree, P, Q)


def test_incremental_add_points_and_repeatability(gpu):
    rs = np.random.default_rng(10)
    parts = [rs.random((n, 3), dtype=f32) for n in (1, 5000, 1234, 20000)]
    inc = K.KdTree(parts[0])
    for p in parts[1:]:
        inc.AddPoints(p)
    allp = np.concatenate(parts)
    one = K.KdTree(allp)
    assert inc.TotalPoints == one.TotalPoints == len(allp)
    Q = rs.random((20_000, 3), dtype=f32)
    a, b, c = inc.SearchMany(Q), one.SearchMany(Q), one.SearchMany(Q)
    for x, y in ((a, b), (b, c)):
        for u, v in zip(x, y):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    _exact(inc, allp, Q)


def test_refusals(gpu):
    with pytest.raises(N.SdfKitNativeError) as e:
        K.KdTree(np.zeros((0, 3), f32))
    assert e.value.status == N.ERR_INVALID
    for bad in (np.nan, np.inf):
        P = np.zeros((10, 3), f32)
        P[4, 1] = bad
        with pytest.raises(N.SdfKitNativeError) as e:
            K.KdTree(P)
        assert e.value.status == N.ERR_INVALID
    tree = K.KdTree(np.zeros((10, 3), f32))
    with pytest.raises(N.SdfKitNativeError) as e:
        tree.AddPoints(np.array([[0, np.nan, 0]], f32))
    assert e.value.status == N.ERR_INVALID and tree.TotalPoints == 10
    icp = K.IterativeClosestPoint(np.eye(3, dtype=f32))
    with pytest.raises(N.SdfKitNativeError) as e:
        icp.RegisterPoints(np.zeros((0, 3), f32))
    assert e.value.status == N.ERR_INVALID


# ---- ICP against the model ----
def _icp_steps_match(static, dynamic, max_iterations=100):
    """Per-iteration totals (the runs limited to k iterations) within 1e-6 of the model's, equal iteration counts."""
    ref_pts = dynamic.copy()
    ref_total, ref_iters, ref_steps = PM.register(static, ref_pts, max_iterations)
    icp = K.IterativeClosestPoint(static)
    model_total = np.eye(4, dtype=f32)
    for k in range(1, ref_iters + 1):
        model_total = Matrix4x4.Multiply(model_total, ref_steps[k - 1])
        icp.MaxIterations = k
        got = icp.RegisterPoints(dynamic.copy())
        assert icp.Iterations == k
        assert np.abs(got - model_total).max() <= 1e-6, (k, got, model_total)
    icp.MaxIterations = max_iterations
    pts = dynamic.copy()
    total = icp.RegisterPoints(pts)
    assert icp.Iterations == ref_iters
    assert np.abs(total - ref_total).max() <= 1e-6
    assert np.abs(pts - ref_pts).max() <= 1e-5
    return ref_iters


def test_icp_random_cloud_against_model(gpu):
    rs = np.random.default_rng(11)
    P = (rs.random((3000, 3), dtype=f32) - f32(0.5))
    xf = Matrix4x4.Multiply(Matrix4x4.CreateRotationY(f32(3.0) * PM.DEG), Matrix4x4.CreateTranslation(f32(0.02), 0, f32(-0.01)))
    iters = _icp_steps_match(P, PM.transform_points(P, xf))
    assert iters >= 2


def test_icp_mesh_vertices_against_model(gpu):
    V = _mesh_vertices("union8", 40)
    xf = Matrix4x4.Multiply(Matrix4x4.CreateRotationX(f32(2.0) * PM.DEG), Matrix4x4.CreateTranslation(0, f32(0.05), 0))
    _icp_steps_match(V, PM.transform_points(V, xf))


def test_icp_device_resident_mesh(gpu):
    """The vertices of a union8 mesh, moved on the device by RotationX(2 deg) * Translation(0, 0.05, 0) (sdfk_mesh_transform),
    registered in place with sdfk_icp_register_device: the inverse comes back within the reference's tolerances."""
    L = N.lib()
    _, sdf = S.CATALOGUE["union8"]()
    m = C.c_void_p()
    n = 64
    N.check(L.sdfk_sample_march(sdf.program(), N.f3([-2.5] * 3), N.f3([2.5] * 3), n, n, n, 0, C.c_float(0.0), 1, C.byref(m)))
    try:
        nv, ni = C.c_int64(), C.c_int64()
        N.check(L.sdfk_mesh_counts(m, C.byref(nv), C.byref(ni)))
        V0 = np.empty((nv.value, 3), f32)
        N.check(L.sdfk_mesh_copy(m, C.c_void_p(V0.ctypes.data), None, None, None))
        expected = Matrix4x4.Multiply(Matrix4x4.CreateRotationX(f32(2.0) * PM.DEG), Matrix4x4.CreateTranslation(0, f32(0.05), 0))
        lin = expected.copy()
        lin[3, :3] = 0
        _, inv_lin = Matrix4x4.Invert(lin)
        nm = np.ascontiguousarray(inv_lin.T)
        N.check(L.sdfk_mesh_transform(m, (C.c_float * 16)(*expected.reshape(-1)), (C.c_float * 16)(*nm.reshape(-1))))
        V1 = np.empty_like(V0)
        N.check(L.sdfk_mesh_copy(m, C.c_void_p(V1.ctypes.data), None, None, None))
        vp = C.c_void_p()
        N.check(L.sdfk_mesh_device_ptrs(m, C.byref(vp), None, None, None))
        icp = K.IterativeClosestPoint(V0)
        inv = icp.RegisterDevicePoints(vp.value, nv.value)
        V2 = np.empty_like(V0)
        N.check(L.sdfk_mesh_copy(m, C.c_void_p(V2.ctypes.data), None, None, None))
    finally:
        L.sdfk_mesh_free(m)
    ok, transform = Matrix4x4.Invert(inv)
    assert ok and 1 <= icp.Iterations < 100
    np.testing.assert_allclose(transform[3, :3], expected[3, :3], rtol=0, atol=1e-4)
    for k in range(3):
        assert abs(float(expected[k, k]) - float(transform[k, k])) <= 1e-6
    np.testing.assert_allclose(V2, V0, rtol=0, atol=1e-4)
    np.testing.assert_allclose(PM.transform_points(V1, inv), V0, rtol=0, atol=1e-4)
    # the same registration from host memory: identical numbers (bitwise reproducible reductions)
    V3 = V1.copy()
    inv_h = K.IterativeClosestPoint(V0).RegisterPoints(V3)
    assert np.array_equal(inv_h, inv) and np.array_equal(V3, V2)


def test_global_register_points_three_clouds(gpu):
    rs = np.random.default_rng(12)
    base = (rs.random((2000, 3), dtype=f32) - f32(0.5))
    moves = [Matrix4x4.CreateTranslation(f32(0.01), 0, 0),
             Matrix4x4.Multiply(Matrix4x4.CreateRotationY(f32(1.0) * PM.DEG), Matrix4x4.CreateTranslation(0, f32(-0.01), 0))]
    clouds = [base.copy()] + [PM.transform_points(base, mv) for mv in moves]
    icp = K.IterativeClosestPoint(base)
    out = icp.GlobalRegisterPoints(clouds)   # (one transform per cloud after the first, as the reference returns)
    assert len(out) == 2
    for c, mv, t in zip(clouds[1:], moves, out):
        np.testing.assert_allclose(c, base, rtol=0, atol=1e-4)
        _, back = Matrix4x4.Invert(t)
        np.testing.assert_allclose(back[3, :3], mv[3, :3], rtol=0, atol=1e-4)
    assert icp.GlobalRegisterPoints([]) == []
    one = icp.GlobalRegisterPoints([base.copy()])
    assert len(one) == 1 and np.array_equal(one[0], np.eye(4, dtype=f32))
    assert icp.StaticTree.TotalPoints == len(base)   # (the two-argument form works on an instance of its own)
