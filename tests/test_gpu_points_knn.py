"""KdTree.SearchKNearest / SearchRadius on the MI355X against the brute-force numpy model (tests/points_knn_model.py).  Every
comparison is bit for bit: indices equal, distances equal as uint32, found / offsets equal."""
import ctypes as C

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from tests import points_knn_model as KM
from tests import points_model as PM
from tests import scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = np.inf


def _u(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _knn_exact(tree, static, queries, k, max_distance=INF):
    idx, dist, found = tree.SearchKNearest(queries, k, max_distance)
    ri, rd, rf = KM.knn(static, queries, k, max_distance)
    assert idx.shape == ri.shape and idx.dtype == np.int32 and dist.dtype == f32 and found.dtype == np.int32
    bad = np.nonzero((idx != ri).any(axis=1))[0]
    assert len(bad) == 0, (k, len(bad), bad[:3], idx[bad[:3]], ri[bad[:3]])
    assert np.array_equal(_u(dist), _u(rd))
    assert np.array_equal(found, rf)
    return idx, dist, found


def _radius_exact(tree, static, queries, r):
    off, idx, dist = tree.SearchRadius(queries, r)
    ro, ri, rd = KM.radius(static, queries, r)
    assert off.dtype == np.int64 and np.array_equal(off, ro)
    assert np.array_equal(idx, ri)
    assert np.array_equal(_u(dist), _u(rd))
    return off, idx, dist


def _mesh_vertices(name, n=48):
    _, sdf = S.CATALOGUE[name]()
    m = sdf.ToMesh([-2.5] * 3, [2.5] * 3, n, n, n, clipToBounds=False)
    return np.ascontiguousarray(np.asarray(m.Vertices, f32).reshape(-1, 3))


@pytest.fixture(scope="module")
def cube(gpu):
    rs = np.random.default_rng(1)
    P = rs.random((20_000, 3), dtype=f32)
    Q = rs.random((4_000, 3), dtype=f32)
    return K.KdTree(P), P, Q


# ---- k nearest ----
@pytest.mark.parametrize("k", [1, 2, 7, 8, 9, 16, 17, 33, 64])
def test_uniform_cube_every_tier(cube, k):
    tree, P, Q = cube
    _, _, found = _knn_exact(tree, P, Q, k)
    assert (found == k).all()


def test_k1_equals_search_many(cube):
    tree, P, Q = cube
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [3e38, 3e38, 3e38], [5, 5, 5]], f32)
    Qb = np.concatenate([Q, bad])
    idx, dist, found = tree.SearchKNearest(Qb, 1)
    si, sd, _ = tree.SearchMany(Qb)
    assert np.array_equal(idx[:, 0], si) and np.array_equal(_u(dist[:, 0]), _u(sd))
    assert np.array_equal(found, (si >= 0).astype(np.int32))


def test_lattice_cell_centres_mass_ties(gpu):
    g = np.arange(12, dtype=f32)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    P = P[np.random.default_rng(4).permutation(len(P))]
    Q = (np.stack(np.meshgrid(g[:-1], g[:-1], g[:-1], indexing="ij"), -1).reshape(-1, 3) + f32(0.5)).astype(f32)
    tree = K.KdTree(P)
    idx8, dist8, _ = _knn_exact(tree, P, Q, 8)
    # the eight corners of the query's cell, in index order
    assert (np.diff(idx8, axis=1) > 0).all() and (dist8 == dist8[:, :1]).all()
    assert (np.abs(P[idx8] - Q[:, None, :]) == f32(0.5)).all()
    idx4, _, _ = _knn_exact(tree, P, Q, 4)
    assert np.array_equal(idx4, idx8[:, :4])   # the four lowest indices
    _knn_exact(tree, P, Q, 27)


def test_duplicates(gpu):
    P = np.tile(np.array([[0.25, -1.0, 3.0]], f32), (1000, 1))
    Q = np.random.default_rng(5).normal(0, 2, (300, 3)).astype(f32)
    tree = K.KdTree(P)
    for k in (3, 40):
        idx, _, _ = _knn_exact(tree, P, Q, k)
        assert (idx == np.arange(k)).all()
    P2 = np.concatenate([np.tile([[0, 0, 0]], (300, 1)), np.tile([[1, 0, 0]], (300, 1))]).astype(f32)
    P2 = P2[np.random.default_rng(6).permutation(600)]
    Q2 = np.concatenate([Q, [[0.5, 0, 0]]]).astype(f32)
    for k in (8, 64):
        _knn_exact(K.KdTree(P2), P2, Q2, k)


def test_three_points_k8(gpu):
    tree = K.KdTree(PM.THREE_POINTS)
    Q = np.array([[0.0, 1.5, 0.0], [0, 0, 0], [2, 2, 2]], f32)
    idx, dist, found = _knn_exact(tree, PM.THREE_POINTS, Q, 8)
    assert (found == 3).all() and (idx[:, 3:] == -1).all() and (dist[:, 3:] == KM.FLT_MAX).all()
    assert idx[0, 0] == 1 and dist[0, 0] == f32(0.5)
    assert list(idx[1, :3]) == [0, 1, 2]   # three ties
    _knn_exact(tree, PM.THREE_POINTS, Q, 20)


def test_degenerate_boxes(gpu):
    rs = np.random.default_rng(7)
    line = np.zeros((5000, 3), f32)
    line[:, 1] = rs.random(5000, dtype=f32)
    plane = np.zeros((5000, 3), f32)
    plane[:, 0], plane[:, 2] = rs.random(5000, dtype=f32), rs.random(5000, dtype=f32)
    point = np.tile(np.array([[1.5, 2.5, -3.5]], f32), (50, 1))
    for P in (line, plane, point):
        Q = rs.normal(0.5, 0.7, (1500, 3)).astype(f32)
        tree = K.KdTree(P)
        for k in (5, 24):
            _knn_exact(tree, P, Q, k)
        _radius_exact(tree, P, Q[:300], 0.4)


def test_outlier_cloud(gpu):
    rs = np.random.default_rng(9)
    P = np.concatenate([rs.random((100_000, 3), dtype=f32), [[1e6, 1e6, 1e6]]]).astype(f32)
    Q = rs.random((500, 3), dtype=f32)
    tree = K.KdTree(P)
    _knn_exact(tree, P, Q, 12)
    _radius_exact(tree, P, Q[:100], 0.03)


@pytest.mark.parametrize("name", ["union8", "colored_spheres"])
def test_mesh_vertices(gpu, name):
    V = _mesh_vertices(name)
    rs = np.random.default_rng(3)
    Q = np.concatenate([V[rs.choice(len(V), 1500)] + rs.normal(0, 0.05, (1500, 3)).astype(f32),
                        rs.uniform(-2.6, 2.6, (1500, 3)).astype(f32)]).astype(f32)
    tree = K.KdTree(V)
    for k in (6, 16, 50):
        _knn_exact(tree, V, Q, k)
    _radius_exact(tree, V, Q[:600], 0.25)


def test_million_points_sampled(gpu):
    rs = np.random.default_rng(2)
    P = (rs.random((1_000_000, 3), dtype=f32) * f32(2) - f32(1))
    Q = (rs.random((200_000, 3), dtype=f32) * f32(2.2) - f32(1.1))
    tree = K.KdTree(P)
    idx, dist, found = tree.SearchKNearest(Q, 16)
    pick = rs.choice(len(Q), 2000, replace=False)
    ri, rd, rf = KM.knn(P, Q[pick], 16)
    assert np.array_equal(idx[pick], ri) and np.array_equal(_u(dist[pick]), _u(rd)) and np.array_equal(found[pick], rf)


def test_nonfinite_and_far_queries(cube):
    tree, P, _ = cube
    rs = np.random.default_rng(8)
    far = (rs.normal(0, 1, (300, 3)) * 1e4).astype(f32)
    same = P[rs.choice(len(P), 300)]
    Q = np.concatenate([far, same]).astype(f32)
    for k in (4, 20):
        _knn_exact(tree, P, Q, k)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 3e38, 3e38]], f32)
    for k in (1, 8, 64):
        idx, dist, found = tree.SearchKNearest(bad, k)
        assert (idx == -1).all() and (dist == KM.FLT_MAX).all() and (found == 0).all()
    off, idx, dist = tree.SearchRadius(bad, INF)
    assert (off == 0).all() and len(idx) == 0 and len(dist) == 0
    _radius_exact(tree, P, np.concatenate([bad, same[:50], far[:50]]), 0.05)


def test_max_distance(cube):
    tree, P, Q = cube
    Q = Q[:600]
    for k, r in ((8, 0.02), (16, 0.05), (64, 0.05), (5, 0.0), (5, 1e-30), (64, 10.0)):
        _knn_exact(tree, P, Q, k, r)
    # the exact-distance pair: included at r = distance, excluded one ulp below
    _, dist, _ = tree.SearchKNearest(Q[:64], 10)
    for i in range(64):
        d = dist[i, 6]
        at = _knn_exact(tree, P, Q[i:i + 1], 10, d)[2][0]
        below = _knn_exact(tree, P, Q[i:i + 1], 10, np.nextafter(d, f32(0)))[2][0]
        assert at == int((dist[i] <= d).sum()) and below == int((dist[i] < d).sum()) and below < at


def test_add_points_then_query_and_repeatability(gpu):
    rs = np.random.default_rng(10)
    parts = [rs.random((n, 3), dtype=f32) for n in (1, 5000, 1234, 20000)]
    inc = K.KdTree(parts[0])
    for p in parts[1:]:
        inc.AddPoints(p)
    allp = np.concatenate(parts)
    one = K.KdTree(allp)
    Q = rs.random((3000, 3), dtype=f32)
    for k in (7, 30):
        a, b, c = inc.SearchKNearest(Q, k), one.SearchKNearest(Q, k), one.SearchKNearest(Q, k)
        for x, y in ((a, b), (b, c)):
            for u, v in zip(x, y):
                assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
        _knn_exact(inc, allp, Q, k)
    a, b, c = inc.SearchRadius(Q, 0.06), one.SearchRadius(Q, 0.06), one.SearchRadius(Q, 0.06)
    for x, y in ((a, b), (b, c)):
        for u, v in zip(x, y):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


# ---- radius ----
def test_radius_csr_on_the_cube(cube):
    tree, P, Q = cube
    # about 0, 10 and 1000 neighbours per query (20 000 points in the unit cube)
    for r, m, lo, hi in ((1e-4, 4000, 0, 0.01), (0.05, 4000, 5, 20), (0.23, 400, 300, 1100)):
        off, _, _ = _radius_exact(tree, P, Q[:m], r)
        mean = off[-1] / m
        assert lo <= mean <= hi, (r, mean)


def test_radius_infinite_on_a_small_set(gpu):
    rs = np.random.default_rng(11)
    P = rs.normal(0, 1, (300, 3)).astype(f32)
    Q = np.concatenate([rs.normal(0, 1, (40, 3)).astype(f32), [[np.nan, 0, 0]], P[:3]]).astype(f32)
    off, idx, _ = _radius_exact(K.KdTree(P), P, Q, INF)
    assert list(np.diff(off)) == [300] * 40 + [0] + [300] * 3
    assert sorted(idx[:300]) == list(range(300))


def test_radius_zero_on_duplicates_of_the_query(gpu):
    P = np.array([[0.5, 0.25, 2], [1, 1, 1], [0.5, 0.25, 2], [3, 3, 3]], f32)
    off, idx, dist = _radius_exact(K.KdTree(P), P, np.array([[0.5, 0.25, 2], [1, 1, 1.5]], f32), 0.0)
    assert list(off) == [0, 2, 2] and list(idx) == [0, 2] and list(dist) == [0, 0]


def test_radius_prefix_equals_knn(cube):
    tree, P, Q = cube
    Q = Q[:800]
    r = 0.1
    off, ri, rd = tree.SearchRadius(Q, r)
    for k in (1, 8, 40, 64):
        idx, dist, found = tree.SearchKNearest(Q, k, r)
        n = np.minimum(k, np.diff(off))
        assert np.array_equal(found, n.astype(np.int32))
        for i in range(len(Q)):
            assert np.array_equal(idx[i, :n[i]], ri[off[i]:off[i] + n[i]]) and np.array_equal(_u(dist[i, :n[i]]), _u(rd[off[i]:off[i] + n[i]]))
            assert (idx[i, n[i]:] == -1).all() and (dist[i, n[i]:] == KM.FLT_MAX).all()
    assert (np.diff(off) > 64).any() and (np.diff(off) < 40).any()


def test_radius_exact_distance_pair(cube):
    tree, P, Q = cube
    _, dist, _ = tree.SearchKNearest(Q[:40], 12)
    for i in range(40):
        d = dist[i, 9]
        at = _radius_exact(tree, P, Q[i:i + 1], d)[0][1]
        below = _radius_exact(tree, P, Q[i:i + 1], np.nextafter(d, f32(0)))[0][1]
        assert below == int((dist[i] < d).sum()) and at > below   # (the point at d itself is in at r = d, out one ulp below)


# ---- the device entry points ----
def test_device_entry_points_on_torch_buffers(cube):
    import torch
    tree, P, Q = cube
    L = N.lib()
    N.bind_torch_stream()
    dev = torch.device("cuda:0")
    n = len(Q)
    Qd = torch.from_numpy(Q).to(dev)

    def p(t):
        return C.c_void_p(t.data_ptr())

    def sync():
        N.check(L.sdfk_synchronize())
        torch.cuda.synchronize()
    for k in (5, 32):
        idx = torch.full((n, k), 7, dtype=torch.int32, device=dev)
        dist = torch.zeros((n, k), dtype=torch.float32, device=dev)
        found = torch.zeros(n, dtype=torch.int32, device=dev)
        N.check(L.sdfk_points_knn_device(tree.handle, p(Qd), n, k, 0.07, p(idx), p(dist), p(found)))
        sync()
        ri, rd, rf = KM.knn(P, Q, k, 0.07)
        assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(_u(dist.cpu().numpy()), _u(rd)) and np.array_equal(found.cpu().numpy(), rf)
        # any output may be NULL
        found2 = torch.zeros(n, dtype=torch.int32, device=dev)
        N.check(L.sdfk_points_knn_device(tree.handle, p(Qd), n, k, 0.07, None, None, p(found2)))
        sync()
        assert np.array_equal(found2.cpu().numpy(), rf)
    r = 0.06
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    N.check(L.sdfk_points_radius_count_device(tree.handle, p(Qd), n, r, p(off)))
    sync()
    ro, ri, rd = KM.radius(P, Q, r)
    assert np.array_equal(off.cpu().numpy(), ro)
    total = int(off[-1].item())
    idx = torch.full((total + 16,), -5, dtype=torch.int32, device=dev)
    dist = torch.full((total + 16,), -5.0, dtype=torch.float32, device=dev)
    N.check(L.sdfk_points_radius_fill_device(tree.handle, p(Qd), n, r, p(off), p(idx), p(dist)))
    sync()
    assert np.array_equal(idx.cpu().numpy()[:total], ri) and np.array_equal(_u(dist.cpu().numpy()[:total]), _u(rd))
    assert (idx.cpu().numpy()[total:] == -5).all() and (dist.cpu().numpy()[total:] == -5.0).all()   # nothing beyond the total
    # without a distance array: the same indices
    idx2 = torch.full((total,), -5, dtype=torch.int32, device=dev)
    N.check(L.sdfk_points_radius_fill_device(tree.handle, p(Qd), n, r, p(off), p(idx2), None))
    sync()
    assert np.array_equal(idx2.cpu().numpy(), ri)
    N.check(L.sdfk_set_stream(None))


def test_host_fill_without_distances_and_null_outputs(cube):
    tree, P, Q = cube
    L = N.lib()
    Q = np.ascontiguousarray(Q[:500])
    r = 0.07
    ro, ri, _ = KM.radius(P, Q, r)
    off = np.zeros(len(Q) + 1, np.int64)
    N.check(L.sdfk_points_radius_count(tree.handle, Q.ctypes.data, len(Q), r, off.ctypes.data))
    assert np.array_equal(off, ro)
    idx = np.empty(int(off[-1]), np.int32)
    N.check(L.sdfk_points_radius_fill(tree.handle, Q.ctypes.data, len(Q), r, off.ctypes.data, idx.ctypes.data, None))
    assert np.array_equal(idx, ri)
    dist = np.empty((len(Q), 9), f32)
    N.check(L.sdfk_points_knn(tree.handle, Q.ctypes.data, len(Q), 9, np.inf, None, dist.ctypes.data, None))
    assert np.array_equal(_u(dist), _u(KM.knn(P, Q, 9)[1]))
    # no queries
    o, i, d = tree.SearchRadius(np.zeros((0, 3), f32), 1.0)
    assert list(o) == [0] and len(i) == 0 and len(d) == 0
    i, d, f = tree.SearchKNearest(np.zeros((0, 3), f32), 3)
    assert i.shape == (0, 3) and d.shape == (0, 3) and f.shape == (0,)


def test_profiled_calls_report_candidates(cube):
    tree, P, Q = cube
    L = N.lib()
    N.check(L.sdfk_profile_enable(1))
    try:
        seen = []
        tree.SearchKNearest(Q, 1)
        seen.append(tree.stats())
        tree.SearchKNearest(Q[:1000], 64)
        seen.append(tree.stats())
        tree.SearchRadius(Q[:500], 0.1)
        seen.append(tree.stats())   # (the fill's)
    finally:
        N.check(L.sdfk_profile_enable(0))
    assert [s["queries"] for s in seen] == [len(Q), 1000, 500]
    per_query = [s["candidates"] / s["queries"] for s in seen]
    assert 1 <= per_query[0] < per_query[1] and per_query[1] >= 64 and per_query[2] > 20_000 * 4.18 * 0.1 ** 3 * 0.5


def _candidates_of_search_and_k1(tree, queries):
    L = N.lib()
    N.check(L.sdfk_profile_enable(1))
    try:
        tree.SearchMany(queries)
        search = tree.stats()
        tree.SearchKNearest(queries, 1)
        knn = tree.stats()
    finally:
        N.check(L.sdfk_profile_enable(0))
    print("candidates / queries: SearchMany", search["candidates"], search["queries"], " SearchKNearest(k=1)", knn["candidates"], knn["queries"])
    assert search["queries"] == knn["queries"] == len(queries)
    return search["candidates"], knn["candidates"]


def test_search_and_k1_walk_the_same_candidates(cube):
    """One shell walk and one stopping rule serve both kernels: on the cube's queries and its four bad queries SearchMany and
    SearchKNearest(k = 1) report the same candidates.  (3e38, 3e38, 3e38), whose d2 to every point overflows, is the query
    that tells: a search without the k-nearest rule's FLT_MAX bound walks all 20 000 points for it.)"""
    tree, P, Q = cube
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [3e38, 3e38, 3e38], [5, 5, 5]], f32)
    search, knn = _candidates_of_search_and_k1(tree, np.concatenate([Q, bad]))
    assert search == knn and search >= len(Q)


def test_host_search_and_knn_with_null_outputs(cube):
    """Any subset of the outputs of the staged host forms: what was asked for equals the call with every output, bitwise."""
    tree, P, Q = cube
    L = N.lib()
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [3e38, 3e38, 3e38], [5, 5, 5]], f32)
    Qb = np.ascontiguousarray(np.concatenate([Q[:997], bad]))
    n, k = len(Qb), 9

    def call(entry, extra, shapes, want):
        outs = [np.full(shape, 7, dtype) if w else None for (shape, dtype), w in zip(shapes, want)]
        N.check(entry(tree.handle, Qb.ctypes.data, n, *extra, *[o.ctypes.data if o is not None else None for o in outs]))
        return outs

    for entry, extra, shapes in ((L.sdfk_points_search, (), [((n,), np.int32), ((n,), f32), ((n, 3), f32)]),
                                 (L.sdfk_points_knn, (k, np.inf), [((n, k), np.int32), ((n, k), f32), ((n,), np.int32)])):
        full = call(entry, extra, shapes, (True, True, True))
        assert (full[0][-4:-1] == -1).all() and (full[0][:-4] >= 0).all()   # (the call compared against did its work)
        for want in ((True, False, False), (False, True, False), (True, True, False), (False, False, False)):
            got = call(entry, extra, shapes, want)
            for g, f, w in zip(got, full, want):
                assert (g is None) == (not w)
                if w:
                    assert np.array_equal(g.view(np.uint8), f.view(np.uint8))


# ---- refusals ----
def test_refusals(cube):
    tree, P, Q = cube
    L = N.lib()
    for k in (0, 65, -1):
        assert L.sdfk_points_knn(tree.handle, Q.ctypes.data, 4, k, np.inf, None, None, None) == N.ERR_INVALID
        assert L.sdfk_points_knn_device(tree.handle, Q.ctypes.data, 4, k, np.inf, None, None, None) == N.ERR_INVALID
    for k in (65, 0, -1):   # the same refusal through the Python layer
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.SearchKNearest(Q[:4], k)
        assert e.value.status == N.ERR_INVALID
    off = np.array([0, 3, 2, 5, 5], np.int64)   # offsets that do not ascend / do not start at 0: the host fill refuses them
    idx = np.zeros(8, np.int32)
    assert L.sdfk_points_radius_fill(tree.handle, Q.ctypes.data, 4, 0.05, off.ctypes.data, idx.ctypes.data, None) == N.ERR_INVALID
    off = np.array([1, 2, 3, 4, 5], np.int64)
    assert L.sdfk_points_radius_fill(tree.handle, Q.ctypes.data, 4, 0.05, off.ctypes.data, idx.ctypes.data, None) == N.ERR_INVALID
    with pytest.raises(N.SdfKitNativeError) as e:   # a bad k is refused whatever the number of queries
        tree.SearchKNearest(np.zeros((0, 3), f32), 65)
    assert e.value.status == N.ERR_INVALID
    for r in (-1.0, np.nan, -np.inf):
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.SearchRadius(Q[:4], r)
        assert e.value.status == N.ERR_INVALID
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.SearchKNearest(Q[:4], 3, r)
        assert e.value.status == N.ERR_INVALID
        off = np.zeros(5, np.int64)
        idx = np.zeros(8, np.int32)
        assert L.sdfk_points_radius_fill(tree.handle, Q.ctypes.data, 4, r, off.ctypes.data, idx.ctypes.data, None) == N.ERR_INVALID
        assert L.sdfk_points_radius_count_device(tree.handle, Q.ctypes.data, 4, r, off.ctypes.data) == N.ERR_INVALID
    off = np.zeros(5, np.int64)
    q = Q.ctypes.data
    assert L.sdfk_points_knn(None, q, 4, 3, np.inf, None, None, None) == N.ERR_INVALID          # null handle
    assert L.sdfk_points_knn_device(None, q, 4, 3, np.inf, None, None, None) == N.ERR_INVALID
    assert L.sdfk_points_radius_count(None, q, 4, 1.0, off.ctypes.data) == N.ERR_INVALID
    assert L.sdfk_points_radius_fill(None, q, 4, 1.0, off.ctypes.data, None, None) == N.ERR_INVALID
    assert L.sdfk_points_radius_count(tree.handle, q, 4, 1.0, None) == N.ERR_INVALID           # null offsets
    assert L.sdfk_points_radius_count(tree.handle, None, 4, 1.0, off.ctypes.data) == N.ERR_INVALID   # null queries
    assert L.sdfk_points_knn(tree.handle, q, -1, 3, np.inf, None, None, None) == N.ERR_INVALID
    # the set still answers
    _knn_exact(tree, P, Q[:50], 3)
