"""KdTree.Clusters / SelectClusters / RemoveSmallClusters / LargestCluster on the MI355X (csrc/lib_points_cluster.hip) against the
numpy model (tests/points_cluster_model.py): labels, sizes, core, counts and n_clusters equal with np.array_equal in the host and
the device form, twice in a row; the counts the model gave are those recorded in tests/golden/points_cluster_cases.json.  The
clouds (tests/points_cluster_cases.py) are the smallest at which the rounds, the border rule and the sizes can go wrong: a border
that is not empty, a tie between two clusters in three index orders, the deepest forest, duplicates and both extreme radii, a
cloud where rounding makes duplicates, and two sheets over many blocks whose waves mix clusters."""
import ctypes as C

import numpy as np
import pytest

from sdfkit_amd import _native as N
from sdfkit_amd.points import KdTree
from tests import points_cluster_cases as CC
from tests import points_cluster_model as CM

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = np.inf
GOLD = CC.golden()


def cluster_host(tree, radius, min_points):
    n = tree.TotalPoints
    labels, sizes = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    core, counts = np.full(n, 7, np.uint8), np.full(n, -7, np.int32)
    c = C.c_int64(-7)
    st = (C.c_int64 * 6)(*[-7] * 6)
    p = lambda a: C.c_void_p(a.ctypes.data)
    N.check(N.lib().sdfk_points_cluster(tree.handle, float(f32(radius)), int(min_points), p(labels), p(sizes), p(core), p(counts), C.byref(c), st))
    assert (sizes[c.value:] == -7).all()                                   # entries from C on are left alone
    return {"labels": labels, "sizes": sizes[:c.value], "core": core, "counts": counts, "n_clusters": c.value, "stats": list(st)}


def cluster_device(tree, radius, min_points):
    import torch
    n = tree.TotalPoints
    N.bind_torch_stream()
    try:
        dev = torch.device("cuda:0")
        labels, sizes = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)
        core, counts = torch.full((n,), 7, dtype=torch.uint8, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        c = C.c_int64(-7)
        st = (C.c_int64 * 6)(*[-7] * 6)
        d = lambda t: C.c_void_p(t.data_ptr())
        N.check(N.lib().sdfk_points_cluster_device(tree.handle, float(f32(radius)), int(min_points), d(labels), d(sizes), d(core), d(counts),
                                                   C.byref(c), st))
        # (the call has finished when it returns)
        labels, sizes, core, counts = labels.cpu().numpy(), sizes.cpu().numpy(), core.cpu().numpy(), counts.cpu().numpy()
    finally:
        N.check(N.lib().sdfk_set_stream(None))
    assert (sizes[c.value:] == -7).all()
    return {"labels": labels, "sizes": sizes[:c.value], "core": core, "counts": counts, "n_clusters": c.value, "stats": list(st)}


def check(P, radius, min_points, tree=None, rows=None, recorded=None):
    """Host form twice, device form, the Python member: all equal to the model.  -> (the model's result, the tree)."""
    want = CM.cluster(P, radius, min_points, rows)
    if recorded is not None:
        assert want["stats"] == recorded["stats"], (want["stats"], recorded)
    return check_against(want, P, radius, min_points, tree)


def check_against(want, P, radius, min_points, tree=None):
    """check, against a result of the model that the caller has already."""
    tree = tree or KdTree(P)
    n = len(P)
    for got in (cluster_host(tree, radius, min_points), cluster_host(tree, radius, min_points), cluster_device(tree, radius, min_points)):
        assert got["n_clusters"] == want["n_clusters"]
        assert np.array_equal(got["counts"], want["counts"])
        assert np.array_equal(got["core"], want["core"].astype(np.uint8))
        assert np.array_equal(got["labels"], want["labels"])
        assert np.array_equal(got["sizes"], want["sizes"])
        assert got["stats"][:4] == want["stats"]
        assert 1 <= got["stats"][4] <= n + 1 and got["stats"][5] >= 0      # (diagnostics: within their bounds, compared with nothing)
    stats = {}
    labels, sizes, core, counts = tree.Clusters(radius, min_points, stats)
    assert core.dtype == bool and np.array_equal(core, want["core"]) and np.array_equal(labels, want["labels"])
    assert np.array_equal(sizes, want["sizes"]) and np.array_equal(counts, want["counts"])
    assert [stats["clusters"], stats["core"], stats["border"], stats["noise"]] == want["stats"]
    return want, tree


# ---- cloud A ----
@pytest.fixture(scope="module")
def cloud_a(gpu):
    P, which = CC.cloud_a()
    return P, which, KdTree(P)


@pytest.mark.parametrize("radius,min_points", CC.A_CASES)
def test_cloud_a(cloud_a, radius, min_points):
    P, which, tree = cloud_a
    want, _ = check(P, radius, min_points, tree, recorded=GOLD["cloud_a"][f"{radius},{min_points}"])
    if (radius, min_points) == (0.2, 1):
        assert want["n_clusters"] == 43 and sorted(want["sizes"])[-3:] == [300, 700, 1500] and (np.sort(want["sizes"])[:40] == 1).all()
    elif (radius, min_points) == (0.2, 6):
        assert want["stats"] == [3, 2500, 0, 40] and (want["labels"][which == 3] == -1).all()
    else:
        assert want["stats"] == [42, 938, 617, 985]                        # a border that is not empty


# ---- the tie ----
@pytest.mark.parametrize("order", [0, 1, 2])
def test_a_border_point_between_two_clusters_follows_the_lower_index(gpu, order):
    name, P, labels, sizes = CC.tie_clouds()[order]
    want, _ = check(P, 1.0, 4)
    origin = int(np.flatnonzero((P == 0).all(axis=1))[0])
    assert want["counts"][origin] == 3 and not want["core"][origin] and want["n_clusters"] == 2     # L and R stay apart
    assert list(want["labels"]) == labels and list(want["sizes"]) == sizes == [5, 4], name
    assert labels == [[0, 0, 0, 0, 1, 1, 1, 1, 0], [0, 0, 0, 0, 1, 1, 1, 1, 0], [0, 0, 0, 0, 0, 1, 1, 1, 1]][order]


# ---- a chain ----
def test_a_chain_is_the_deepest_forest(gpu):
    P = CC.chain()
    n = len(P)
    tree = KdTree(P)
    rows = CM.neighbours(P, 1.0)
    want, _ = check(P, 1.0, 1, tree, rows, GOLD["chain"]["1,1"])
    assert want["n_clusters"] == 1 and list(want["sizes"]) == [n]
    want, _ = check(P, CC.BELOW_ONE, 1, tree, recorded=GOLD["chain"]["below_1,1"])
    assert want["n_clusters"] == n and (want["sizes"] == 1).all() and np.array_equal(want["labels"], np.arange(n))
    want, _ = check(P, 1.0, 3, tree, rows, GOLD["chain"]["1,3"])
    assert want["stats"] == [1, n - 2, 2, 0]


# ---- duplicates and extremes ----
def test_duplicates_and_both_extreme_radii(gpu):
    P = CC.duplicates()
    tree = KdTree(P)
    g = GOLD["duplicates"]
    assert check(P, 0.0, 1, tree, recorded=g["0.0,1"])[0]["stats"] == [9, 19, 0, 0]
    assert check(P, 0.0, 3, tree, recorded=g["0.0,3"])[0]["stats"] == [5, 15, 0, 4]
    assert check(P, 0.0, 4, tree, recorded=g["0.0,4"])[0]["stats"] == [0, 0, 0, 19]      # n_clusters = 0: sizes untouched (cluster_host asserts)
    assert check(P, INF, 1, tree, recorded=g["inf,1"])[0]["stats"] == [1, 19, 0, 0]
    assert check(P, INF, 20, tree, recorded=g["inf,20"])[0]["stats"] == [0, 0, 0, 19]
    one = np.array([[0.25, -3, 7]], f32)
    assert check(one, 0.5, 1)[0]["stats"] == [1, 1, 0, 0]
    assert check(one, 0.0, 2)[0]["stats"] == [0, 0, 0, 1]


def test_null_outputs_and_refusals(gpu):
    P, _ = CC.cloud_a()
    P = P[:400]
    tree = KdTree(P)
    n = len(P)
    want = CM.cluster(P, 0.3, 3)
    p = lambda a: C.c_void_p(a.ctypes.data)
    # any output may be NULL: labels alone, then the count alone
    labels = np.full(n, -7, np.int32)
    N.check(N.lib().sdfk_points_cluster(tree.handle, 0.3, 3, p(labels), None, None, None, None, None))
    assert np.array_equal(labels, want["labels"])
    c = C.c_int64(-7)
    N.check(N.lib().sdfk_points_cluster(tree.handle, 0.3, 3, None, None, None, None, C.byref(c), None))
    assert c.value == want["n_clusters"]
    # refusals leave everything as it was
    sizes, core, counts = np.full(n, -7, np.int32), np.full(n, 7, np.uint8), np.full(n, -7, np.int32)
    labels[:] = -7
    st = (C.c_int64 * 6)(*[-7] * 6)
    c = C.c_int64(-7)
    for radius, mp in ((-1.0, 1), (np.nan, 1), (-INF, 1), (0.5, 0), (0.5, -3)):
        for entry in (N.lib().sdfk_points_cluster, N.lib().sdfk_points_cluster_device):      # (refused before any pointer is used)
            assert entry(tree.handle, float(radius), mp, p(labels), p(sizes), p(core), p(counts), C.byref(c), st) == N.ERR_INVALID
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.Clusters(radius, mp)
        assert e.value.status == N.ERR_INVALID
    assert N.lib().sdfk_points_cluster(None, 0.5, 1, p(labels), p(sizes), p(core), p(counts), C.byref(c), st) == N.ERR_INVALID
    assert (labels == -7).all() and (sizes == -7).all() and (core == 7).all() and (counts == -7).all() and c.value == -7 and list(st) == [-7] * 6
    k = C.c_int64(-7)
    idx = np.full(n, -7, np.int32)
    keep = np.ones(4, np.uint8)
    for args in ((None, p(labels), p(keep), 4), (tree.handle, None, p(keep), 4), (tree.handle, p(labels), p(keep), -1), (tree.handle, p(labels), None, 4)):
        assert N.lib().sdfk_points_select(*args, p(idx), None, C.byref(k)) == N.ERR_INVALID
    assert (idx == -7).all() and k.value == -7


# ---- a far cloud ----
def test_a_far_cloud_where_rounding_makes_duplicates(gpu):
    P = CC.far_cloud()
    assert len(np.unique(P, axis=0)) < len(P)
    tree = KdTree(P)
    check(P, 0.25, 1, tree, recorded=GOLD["far"]["0.25,1"])
    want, _ = check(P, 0.5, 4, tree, recorded=GOLD["far"]["0.5,4"])
    assert want["n_clusters"] == 1 and list(want["sizes"]) == [600]


# ---- two sheets ----
@pytest.fixture(scope="module")
def sheets(gpu):
    P, sheet = CC.two_sheets()
    return P, sheet, KdTree(P), {}


@pytest.mark.parametrize("radius,min_points", CC.SHEET_CASES)
def test_two_sheets_over_many_blocks(sheets, radius, min_points):
    P, sheet, tree, rows = sheets
    if radius not in rows:
        rows[radius] = CM.neighbours(P, radius)
    want, _ = check(P, radius, min_points, tree, rows[radius], GOLD["two_sheets"][f"{radius},{min_points}"])
    if radius == 0.31:
        assert want["n_clusters"] == 1 and list(want["sizes"]) == [20_000] and 150 < want["counts"].mean() < 230
    else:
        assert want["n_clusters"] == 2
        kept = want["labels"] >= 0
        first = sheet[np.flatnonzero(want["core"])[0]]
        assert np.array_equal(want["labels"][kept], (sheet != first).astype(np.int32)[kept])      # a sheet each, numbered by the lowest core member
        if min_points == 1:
            assert list(want["sizes"]) == [10_000, 10_000]
        else:
            assert 12 <= want["stats"][2] <= 120                           # a few dozen border points


# ---- select ----
def select_device(tree, labels, keep):
    import torch
    n = tree.TotalPoints
    N.bind_torch_stream()
    try:
        dev = torch.device("cuda:0")
        lab = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(dev)
        kp = torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).to(dev)
        idx, pts = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        k = C.c_int64(-7)
        N.check(N.lib().sdfk_points_select_device(tree.handle, C.c_void_p(lab.data_ptr()), C.c_void_p(kp.data_ptr()) if len(keep) else None, len(keep),
                                                  C.c_void_p(idx.data_ptr()), C.c_void_p(pts.data_ptr()), C.byref(k)))
        idx, pts = idx.cpu().numpy(), pts.cpu().numpy()
    finally:
        N.check(N.lib().sdfk_set_stream(None))
    assert (idx[k.value:] == -7).all() and (pts[k.value:] == -7).all()      # entries from n_kept on are left alone
    return pts[:k.value], idx[:k.value]


def check_select(tree, P, labels, keep):
    want = CM.select(labels, keep)
    for pts, idx in (tree.SelectClusters(labels, keep), select_device(tree, labels, np.asarray(keep).astype(np.uint8))):
        assert np.array_equal(idx, want) and np.array_equal(pts.view(np.uint32), P[want].view(np.uint32))
    return want


def test_select_by_size_and_the_conveniences(cloud_a):
    P, which, tree = cloud_a
    want = CM.cluster(P, 0.2, 1)
    for min_size in (1, 2, 301, 701, 1501):
        keep = CM.keep_by_size(want["sizes"], min_size)
        kept = check_select(tree, P, want["labels"], keep)
        assert np.array_equal(kept, np.flatnonzero(keep[want["labels"]].astype(bool)))
    # RemoveSmallClusters drops the strays and keeps the three spheres
    stats = {}
    pts, idx, labels = tree.RemoveSmallClusters(0.2, 1, 2, stats)
    assert len(idx) == 2500 and np.array_equal(idx, np.flatnonzero(which != 3)) and np.array_equal(labels, want["labels"]) and stats["clusters"] == 43
    assert np.array_equal(pts.view(np.uint32), P[idx].view(np.uint32))
    # ... with minPoints = 6 the strays are noise, and noise goes whatever minSize is
    pts, idx, labels = tree.RemoveSmallClusters(0.2, 6, 1)
    assert len(idx) == 2500 and (labels[which == 3] == -1).all()
    # LargestCluster: the sphere of 1500
    pts, idx = tree.LargestCluster(0.2, 1)
    assert np.array_equal(idx, np.flatnonzero(which == 0)) and CM.largest(want["sizes"]) == want["labels"][idx[0]]
    # a KdTree made from the result clusters into the same sizes
    pts, idx, _ = tree.RemoveSmallClusters(0.2, 1, 2)
    again = KdTree(pts).Clusters(0.2, 1)
    assert sorted(again[1]) == [300, 700, 1500] and (again[0] >= 0).all()


def test_largest_cluster_tie_goes_to_the_lowest_number(gpu):
    P = np.array([[5, 0, 0], [0, 0, 0], [5.1, 0, 0], [0.1, 0, 0], [9, 9, 9]], f32)
    tree = KdTree(P)
    labels, sizes, _, _ = tree.Clusters(0.5, 1)
    assert list(labels) == [0, 1, 0, 1, 2] and list(sizes) == [2, 2, 1]
    assert list(tree.LargestCluster(0.5, 1)[1]) == [0, 2]
    assert len(tree.LargestCluster(0.5, 6)[1]) == 0                         # no cluster at all: nothing


def test_select_with_labels_not_made_by_the_library(cloud_a):
    P, _, tree = cloud_a
    rs = np.random.default_rng(23)
    labels = rs.integers(-3, 9, len(P)).astype(np.int32)                     # negative, and beyond the 5 keep bytes
    labels[:4] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, 5]
    kept = check_select(tree, P, labels, [1, 0, 1, 1, 0])
    assert 0 < len(kept) < len(P) and set(labels[kept]) == {0, 2, 3}
    assert len(check_select(tree, P, labels, [0, 0, 0, 0, 0])) == 0
    assert len(check_select(tree, P, labels, [])) == 0                      # n_clusters = 0 keeps nothing


# ---- profiling ----
def test_a_profiled_call_reports_candidates(cloud_a):
    P, _, tree = cloud_a
    L = N.lib()
    N.check(L.sdfk_profile_enable(1))
    try:
        tree.Clusters(0.2, 1)
        euclid = tree.stats()
        tree.Clusters(0.12, 10)
        dbscan = tree.stats()
    finally:
        N.check(L.sdfk_profile_enable(0))
    want = CM.cluster(P, 0.2, 1)
    assert euclid["queries"] == dbscan["queries"] == len(P)
    assert euclid["candidates"] >= 2 * int(want["counts"].sum()) and dbscan["candidates"] > 0      # the count walk and a hook round at the least
