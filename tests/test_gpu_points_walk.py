"""The KdTree's shell walk (csrc/points_walk.h) on the MI355X on the adversarial clouds of tests/points_cases.py: points within
rounding distance of a cell boundary, clouds far from the origin, scales at which d2 is denormal, zero or infinite, a needle, a
sheet and two clusters with a void between.  Every row of SearchMany, SearchKNearest (the register tier and the three LDS tiers)
and SearchRadius equals the brute-force models bit for bit, and the candidates a profiled call reports equal the numpy restatement
of the walk (points_cases.Walk) exactly: that pins the lower bound and the stopping rule themselves -- a device that walks a shell
short and gets lucky fails, and so does one that walks too far."""
import numpy as np
import pytest

from sdfkit_amd import _native as N
from sdfkit_amd.points import KdTree
from tests import points_cases as PC
from tests import points_knn_model as KM
from tests import points_model as PM

pytestmark = pytest.mark.gpu
f32 = np.float32
KS = (1, 8, 9, 33, 64)      # the register tier at its edge, and the LDS tiers 16, 64 and 64 full

_trees = {}


def _tree(name):
    if name not in _trees:
        _trees[name] = KdTree(PC.case(name)[0])
    return _trees[name]


def _u(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _rows_differ(got, want):
    """The number of queries whose row differs (bits for f32)."""
    g, w = (_u(got), _u(want)) if want.dtype == f32 else (got, want)
    assert g.shape == w.shape
    return int((g != w).reshape(len(g), -1).any(axis=1).sum())


@pytest.mark.parametrize("name", PC.NAMES)
def test_rows_equal_brute_force(gpu, name):
    P, Q = PC.case(name)
    tree = _tree(name)
    assert tuple(tree.stats()["grid"]) == tuple(PC.walk_of(name).G["dim"])
    got = tree.SearchMany(Q)
    want = PM.nearest(P, Q)
    bad = [_rows_differ(g, w) for g, w in zip(got, want)]
    print(name, "SearchMany: rows that differ (index, distance, nearest)", bad, "not found", int((want[0] < 0).sum()))
    assert bad == [0, 0, 0]
    for k in KS:
        got = tree.SearchKNearest(Q, k)
        want = KM.knn(P, Q, k)
        bad = [_rows_differ(g, w) for g, w in zip(got, want)]
        print(name, "SearchKNearest", k, ": rows that differ (index, distance, found)", bad)
        assert bad == [0, 0, 0]
    r = PC.radius_of(name)
    off, idx, dist = tree.SearchRadius(Q, r)
    ro, ri, rd = KM.radius(P, Q, r)
    print(name, "SearchRadius", float(r), ":", int(off[-1]), "neighbours, the model", int(ro[-1]))
    assert np.array_equal(off, ro) and np.array_equal(idx, ri) and np.array_equal(_u(dist), _u(rd))
    traps = PC.trap_queries(name)
    if traps:
        assert traps[0] >= 8 and np.array_equal(tree.SearchMany(Q[:traps[0]])[0], traps[1])


@pytest.mark.parametrize("name", PC.NAMES)
def test_candidates_equal_the_walk_model(gpu, name):
    """sdfk_profile_enable(1): the candidates of SearchMany and of SearchKNearest(k = 8) over the case's queries, against the
    restated walk's for k = 1 and k = 8."""
    _, Q = PC.case(name)
    tree = _tree(name)
    want = [int(PC.answers(name, k)[3].sum()) for k in (1, 8)]
    walked = max(1, int(np.isfinite(Q).all(axis=1).sum()))
    L = N.lib()
    N.check(L.sdfk_profile_enable(1))
    try:
        tree.SearchMany(Q)
        search = tree.stats()
        tree.SearchKNearest(Q, 8)
        knn = tree.stats()
    finally:
        N.check(L.sdfk_profile_enable(0))
    print(name, "candidates: SearchMany", search["candidates"], "model", want[0], f"({want[0] / walked:.1f} per query);  SearchKNearest(8)",
          knn["candidates"], "model", want[1], f"({want[1] / walked:.1f} per query)")
    assert search["queries"] == knn["queries"] == len(Q)
    assert [search["candidates"], knn["candidates"]] == want


def test_overflowing_scales(gpu):
    """scale_100: every d2 but 0 overflows, so no query finds a point but the static points asked for themselves (distance 0; every
    case asks those) -- and the walk gives up after its first shells.  scale_64: found is as the model says, some and not all."""
    P, Q = PC.case("scale_100")
    idx, dist, _ = _tree("scale_100").SearchMany(Q)
    own = (Q[:, None, :] == P[None, :, :]).all(axis=2).any(axis=1)
    assert (idx[~own] == -1).all() and (dist[~own] == PC.FLT_MAX).all() and (~own).sum() > 150
    assert (idx[own] >= 0).all() and (dist[own] == 0).all()
    i8, _, f8 = _tree("scale_100").SearchKNearest(Q, 8)
    assert (i8[~own] == -1).all() and (f8[~own] == 0).all()
    P, Q = PC.case("scale_64")
    found = _tree("scale_64").SearchKNearest(Q, 8)[2]
    want = KM.knn(P, Q, 8)[2]
    assert np.array_equal(found, want) and (want == 8).any() and (want == 0).any()


@pytest.mark.parametrize("name", ["far4096", "far65536"])
def test_far_cloud_outliers(gpu, name):
    from tests.test_gpu_points_filter import check_outliers
    want = check_outliers(PC.case(name)[0], 8, 2.0)
    assert want["stats"][0] > 3000


@pytest.mark.parametrize("name", ["far4096", "far65536"])
def test_far_cloud_normals(gpu, name):
    from tests.test_gpu_pointcloud import _normals_exact
    _normals_exact(_tree(name), PC.case(name)[0], 8)
