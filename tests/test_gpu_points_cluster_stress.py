"""KdTree.Clusters / SelectClusters on the MI355X on the stress cases (tests/points_cluster_stress_cases.py; what each case is there
for is proved from the model alone in tests/test_points_cluster_stress_cases.py) against the numpy model
(tests/points_cluster_model.py), in the host form, the device form and the Python members, by the comparisons of the unit's own
tests, imported from them.  The shuffled clouds of tests/test_gpu_points_cluster.py keep the forest shallow, the waves mixed and
the border ties to two candidates; here are chains whose index order makes the deepest forest and the most hook rounds a path can
need (the rounds the device reports are held against the bound the CPU file proves), a border point between six clusters at one
d2 in 72 layouts, waves laid out lane by lane for the sizes kernel, all sixteen combinations of absent outputs, point counts on
the edges of the scan's blocks and beyond its 256 block totals, squared distances that overflow and underflow binary32, and the
library's own radius query as a second witness of the counts and the border choice.  Everything is an integer (the kept points:
float bits) compared with np.array_equal -- nothing here has a tolerance."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from sdfkit_amd import _native as N
from sdfkit_amd.points import KdTree
from tests import points_cluster_cases as CC
from tests import points_cluster_model as CM
from tests import points_cluster_stress_cases as SC
from tests.test_gpu_points_cluster import check, check_against, check_select, cluster_device, cluster_host

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = np.inf
KEYS = ("labels", "sizes", "core", "counts")


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS) and a["n_clusters"] == b["n_clusters"] and a["stats"] == b["stats"]


# ---- 1. the chains ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.CHAIN_ORDERS)
def test_chains_deep_forests_and_the_most_rounds_of_a_path(gpu, name):
    """One cluster whatever the order of the indices; the hook rounds stay within ceil(log2 n) + 1 = 15 (a degenerate driver, one
    tree a round, would need thousands), and every round flattens within its 64 shortcut launches.  The counts themselves may
    vary from run to run and are compared with nothing."""
    P = SC.chain(name)
    n = len(P)
    tree = KdTree(P)
    bound = math.ceil(math.log2(n)) + 1
    assert bound == 15
    for mp in (1, 3):
        want = SC.chain_expected(P, mp)
        assert want["stats"] == ([1, n, 0, 0] if mp == 1 else [1, n - 2, 2, 0])
        check_against(want, P, 1.0, mp, tree)
        for form in (cluster_host, cluster_device):
            rounds, shortcuts = form(tree, 1.0, mp)["stats"][4:6]
            print(f"chain {name} min_points {mp} {form.__name__}: rounds {rounds} shortcuts {shortcuts}")
            assert 2 <= rounds <= bound, (name, mp, rounds)
            assert 1 <= shortcuts <= 64 * rounds, (name, mp, rounds, shortcuts)


# ---- 2. the star -----------------------------------------------------------------------------------------------------------------
def test_star_a_border_point_between_six_clusters_follows_the_lowest_index(gpu):
    for lay in SC.STAR_LAYOUTS:
        P, radius, centre, inner = SC.star(*lay)
        want = CM.cluster(P, radius, SC.STAR_MIN_POINTS)
        assert want["stats"] == [6, 96, 1, 0] and want["labels"][centre] == SC.STAR_PERMUTATIONS[lay[0]][0] == int(inner.argmin()), lay
        try:
            check_against(want, P, radius, SC.STAR_MIN_POINTS)
        except AssertionError as e:
            raise AssertionError(f"star layout {lay}") from e


# ---- 3. the waves ----------------------------------------------------------------------------------------------------------------
def _raw(tree, form, radius, min_points, present=KEYS, totals=True):
    """One call of the host or the device form with only the outputs in `present` given (the others NULL), n_clusters and stats
    given or both NULL -> (the four buffers as numpy arrays, sentinel-filled where not given; n_clusters; stats)."""
    n = tree.TotalPoints
    bufs = {"labels": np.full(n, -7, np.int32), "sizes": np.full(n, -7, np.int32), "core": np.full(n, 7, np.uint8), "counts": np.full(n, -7, np.int32)}
    c = C.c_int64(-7)
    st = (C.c_int64 * 6)(*[-7] * 6)
    tail = (C.byref(c), st) if totals else (None, None)
    if form == "host":
        args = [C.c_void_p(bufs[k].ctypes.data) if k in present else None for k in KEYS]
        N.check(N.lib().sdfk_points_cluster(tree.handle, float(f32(radius)), int(min_points), *args, *tail))
    else:
        import torch
        N.bind_torch_stream()
        try:
            dev = {k: torch.from_numpy(bufs[k]).to("cuda:0") for k in KEYS}
            torch.cuda.synchronize()
            args = [C.c_void_p(dev[k].data_ptr()) if k in present else None for k in KEYS]
            N.check(N.lib().sdfk_points_cluster_device(tree.handle, float(f32(radius)), int(min_points), *args, *tail))
            bufs = {k: dev[k].cpu().numpy() for k in KEYS}
        finally:
            N.check(N.lib().sdfk_set_stream(None))
    return bufs, c.value, list(st)


def _check_raw(want, got, present, totals, what):
    bufs, c, st = got
    nc = want["n_clusters"]
    for k in KEYS:
        if k not in present:
            assert (bufs[k] == (7 if k == "core" else -7)).all(), (what, k)
        elif k == "sizes":
            assert np.array_equal(bufs[k][:nc], want[k]) and (bufs[k][nc:] == -7).all(), (what, k)     # entries from C on are left alone
        else:
            assert np.array_equal(bufs[k], want[k].astype(bufs[k].dtype)), (what, k)
    if totals:
        assert c == nc and st[:4] == want["stats"] and st[4] >= 1 and st[5] >= 0, (what, c, st)
    else:
        assert c == -7 and st == [-7] * 6, what


def test_waves_laid_out_by_index_with_and_without_sizes(gpu):
    P, border = SC.waves()
    want, tree = check(P, SC.WAVES_RADIUS, SC.WAVES_MIN_POINTS)
    assert np.array_equal(want["labels"], SC.WAVES_LABELS) and want["stats"] == [4, 384, 4, 97] and list(want["sizes"]) == [191, 95, 65, 37]
    for form in ("host", "device"):
        for present in (("labels", "core", "counts"), (), KEYS, ("sizes",)):       # sizes NULL: the totals only
            _check_raw(want, _raw(tree, form, SC.WAVES_RADIUS, SC.WAVES_MIN_POINTS, present), present, True, (form, present))
    pts, idx = tree.LargestCluster(SC.WAVES_RADIUS, SC.WAVES_MIN_POINTS)
    assert np.array_equal(idx, np.flatnonzero(SC.WAVES_LABELS == SC.A)) and np.array_equal(pts.view(np.uint32), P[idx].view(np.uint32))
    pts, idx, labels = tree.RemoveSmallClusters(SC.WAVES_RADIUS, SC.WAVES_MIN_POINTS, 65)
    assert np.array_equal(idx, np.flatnonzero((SC.WAVES_LABELS == SC.A) | (SC.WAVES_LABELS == SC.B) | (SC.WAVES_LABELS == SC.C_)))
    assert np.array_equal(labels, SC.WAVES_LABELS)
    for keep in ([0, 0, 1, 0], [0, 1, 0, 1], [1, 1, 1, 1], [0, 0, 0, 1]):
        check_select(tree, P, want["labels"], keep)


# ---- 4. absent outputs -----------------------------------------------------------------------------------------------------------
def test_all_sixteen_combinations_of_absent_outputs(gpu):
    P, _ = CC.cloud_a()
    P = P[:400]
    tree = KdTree(P)
    want = CM.cluster(P, 0.3, 3)
    assert want["stats"][2] > 0 and want["stats"][3] > 0 and 1 < want["n_clusters"] < 400
    for form in ("host", "device"):
        for r in range(5):
            for present in itertools.combinations(KEYS, r):
                for totals in (True, False):
                    _check_raw(want, _raw(tree, form, 0.3, 3, present, totals), present, totals, (form, present, totals))


# ---- 5. n on the edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.PAIRS_MODEL_N)
def test_pairs_on_the_edges_of_waves_blocks_and_the_scan(gpu, n):
    P = SC.pairs(n)
    want, tree = check(P, SC.PAIRS_RADIUS, 1, rows=SC.pairs_rows(n))
    assert _same(want, SC.pairs_expected(n, 1)) and want["n_clusters"] == (n + 1) // 2
    kept = check_select(tree, P, want["labels"], SC.pairs_keep(want["n_clusters"]))
    assert np.array_equal(kept, SC.pairs_kept(n))
    if n == 257:                                                                  # the last cluster's label equals the n_clusters given: not kept
        assert list(check_select(tree, P, want["labels"], np.ones(128, np.uint8))) == list(range(256))


def test_pairs_beyond_the_scan_carry(gpu):
    n = SC.PAIRS_LARGE_N
    P = SC.pairs(n)
    tree = KdTree(P)
    for mp in (1, 2, 3):
        want = SC.pairs_expected(n, mp)
        assert want["n_clusters"] == (262_145 if mp <= 2 else 0)                   # (n is even: min_points 2 gives the same answer)
        check_against(want, P, SC.PAIRS_RADIUS, mp, tree)                          # (min_points 3: no cluster, sizes untouched -- cluster_host asserts)
    labels = SC.pairs_expected(n, 1)["labels"]
    keep = SC.pairs_keep(262_145)
    assert np.array_equal(check_select(tree, P, labels, keep), SC.pairs_kept(n))
    kept = check_select(tree, P, labels, 1 - keep)                                 # the opposite bytes keep the last cluster: kept points in the last scan block
    assert list(kept[-2:]) == [n - 2, n - 1]


# ---- 6. d2 beyond binary32 -------------------------------------------------------------------------------------------------------
def test_overflow_and_underflow_of_d2(gpu):
    P, clump = SC.overflow()
    tree = KdTree(P)
    for radius, mp, stats in SC.OVERFLOW_CASES:
        want, _ = check(P, radius, mp, tree)
        assert want["stats"] == stats and (mp > 1 or list(want["sizes"]) == [40, 40]), (radius, mp)
    P, tiny = SC.underflow()
    tree = KdTree(P)
    for radius, mp, stats in SC.UNDERFLOW_CASES:
        want, _ = check(P, radius, mp, tree)
        assert want["stats"] == stats and len(set(want["labels"][tiny])) == 1, (radius, mp)


# ---- 7. the library's own radius query as the witness ----------------------------------------------------------------------------
def _consistent(P, radius, min_points, what):
    tree = KdTree(P)
    labels, sizes, core, counts = tree.Clusters(radius, min_points)
    off, idx, _ = tree.SearchRadius(P, radius)
    assert np.array_equal(counts, np.diff(off).astype(np.int32)), what
    borders = 0
    for i in np.flatnonzero(~core):
        row = idx[off[i]:off[i + 1]]
        hit = row[core[row]]
        assert labels[i] == (labels[hit[0]] if len(hit) else -1), (what, i)
        borders += len(hit) > 0
    return borders


def test_counts_and_border_labels_agree_with_search_radius(gpu):
    for lay in SC.STAR_LAYOUTS:
        if lay[0] == 1:
            P, radius, _, _ = SC.star(*lay)
            assert _consistent(P, radius, SC.STAR_MIN_POINTS, ("star", lay)) == 1
    assert _consistent(SC.waves()[0], SC.WAVES_RADIUS, SC.WAVES_MIN_POINTS, "waves") == 4
    for radius, mp, _ in SC.OVERFLOW_CASES:
        _consistent(SC.overflow()[0], radius, mp, ("overflow", radius, mp))
    for radius, mp, _ in SC.UNDERFLOW_CASES:
        _consistent(SC.underflow()[0], radius, mp, ("underflow", radius, mp))
    _consistent(SC.pairs(4097), SC.PAIRS_RADIUS, 1, "pairs")
    assert _consistent(SC.chain("bit_reversed", 1024), 1.0, 3, "chain") == 2
