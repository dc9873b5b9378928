"""The clustering stress cases (tests/points_cluster_stress_cases.py) against the numpy model alone, on the CPU: every case has the
property it is there for, the closed-form neighbour rows and results equal the model's (and scipy's cKDTree for the one cloud too
large for the model), a simulation of the hook rule of sdfkit_amd/csrc/points_cluster.h bounds the hook rounds of a chain, and
each of twelve named wrong variants of the model -- a few lines over the model's own intermediate arrays, below -- gives a
result that differs from the model's on at least one named case.  What the device does with the cases is
tests/test_gpu_points_cluster_stress.py; a case that lost its property would make that test pass for nothing."""
import functools
import math

import numpy as np
import pytest

from tests import points_cluster_model as CM
from tests import points_cluster_stress_cases as SC
from tests import points_knn_model as KM

f32, f64, i32, i64 = np.float32, np.float64, np.int32, np.int64
INF = np.inf
KEYS = ("labels", "sizes", "core", "counts")


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS) and a["n_clusters"] == b["n_clusters"] and a["stats"] == b["stats"]


def _same_rows(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the named cases the variants run on: name -> (points, radius, min_points, rows or None) ---------------------------------------
STAR_NAMED = (1, "first", 0)                     # arm 3 wins; cluster 0 is the lowest number, arm 0 holds the highest inner index


@functools.lru_cache(maxsize=None)
def _cases():
    out = {}
    for name in SC.CHAIN_ORDERS:
        P = SC.chain(name, 1024)
        for mp in (1, 3):
            out[("chain", name, mp)] = (P, 1.0, mp)
    for lay in SC.STAR_LAYOUTS:
        P, radius, _, _ = SC.star(*lay)
        out[("star",) + lay] = (P, radius, SC.STAR_MIN_POINTS)
    out["waves"] = (SC.waves()[0], SC.WAVES_RADIUS, SC.WAVES_MIN_POINTS)
    for radius, mp, _ in SC.OVERFLOW_CASES:
        out[("overflow", radius, mp)] = (SC.overflow()[0], radius, mp)
    for radius, mp, _ in SC.UNDERFLOW_CASES:
        out[("underflow", radius, mp)] = (SC.underflow()[0], radius, mp)
    for n in (1, 2, 63, 257):
        out[("pairs", n)] = (SC.pairs(n), SC.PAIRS_RADIUS, 1)
    return out


@functools.lru_cache(maxsize=None)
def _model(name):
    P, radius, mp = _cases()[name]
    return CM.cluster(P, radius, mp)


# ---- 1. the chains ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.CHAIN_ORDERS)
def test_chain_rows_in_closed_form_are_the_models(name):
    P = SC.chain(name, 1024)
    assert _same_rows(SC.chain_rows(P), CM.neighbours(P, 1.0))
    assert sorted(P[:, 0].tolist()) == list(range(1024)) and not P[:, 1:].any()
    index_of = SC.chain_order(name, 1024)
    assert np.array_equal(P[index_of, 0], np.arange(1024))
    if name == "bit_reversed":
        assert np.array_equal(index_of[index_of], np.arange(1024)) and index_of[1] == 512 and index_of[3] == 768


@pytest.mark.parametrize("name", SC.CHAIN_ORDERS)
def test_chains_are_one_cluster_and_two_border_ends(name):
    n = SC.CHAIN_N
    P = SC.chain(name)
    rows = SC.chain_rows(P)
    assert len(P) == n == 1 << 14 and len(rows[1]) == 3 * n - 2
    out = CM.cluster(P, 1.0, 1, rows)
    assert out["stats"] == [1, n, 0, 0] and list(out["sizes"]) == [n] and not out["labels"].any()
    assert _same(out, SC.chain_expected(P, 1))
    out = CM.cluster(P, 1.0, 3, rows)
    assert out["stats"] == [1, n - 2, 2, 0] and list(out["sizes"]) == [n]
    assert _same(out, SC.chain_expected(P, 3))                                  # (the device is compared with the closed form: the model's
    #                                                                             own rounds over the bit-reversed chain take seconds)
    ends = np.flatnonzero(~out["core"])
    assert sorted(P[ends, 0].tolist()) == [0, n - 1] and list(out["counts"][ends]) == [2, 2] and (out["labels"] == 0).all()


def hook_rounds(index_of, schedule, rng=None):
    """The hook rounds of points_cluster.h over the path whose node at position x is index_of[x]: on an edge whose ends have the
    parents pi != pj, the lower one is offered to parent[the higher one], which keeps the minimum; then the forest is flattened;
    this repeats until a round changes nothing, and that round counts.  Schedules: `snapshot`, every edge reads the parents as
    they were before the round; `sequential`, the edges one after another in path order, each on the parents as they are;
    `random`, the same in a random order.  -> the number of rounds."""
    n = len(index_of)
    a, b = np.asarray(index_of[:-1], i64), np.asarray(index_of[1:], i64)
    parent = np.arange(n, dtype=i64)
    rounds = 0
    while True:
        rounds += 1
        before = parent.copy()
        if schedule == "snapshot":
            pa, pb = before[a], before[b]
            m = pa != pb
            np.minimum.at(parent, np.maximum(pa, pb)[m], np.minimum(pa, pb)[m])
        else:
            par = parent.tolist()
            for e in (range(n - 1) if schedule == "sequential" else rng.permutation(n - 1).tolist()):
                pi, pj = par[a[e]], par[b[e]]
                if pi != pj:
                    at, offered = max(pi, pj), min(pi, pj)
                    par[at] = min(par[at], offered)
            parent = np.array(par, i64)
        changed = not np.array_equal(parent, before)
        assert np.all(parent <= np.arange(n))
        while True:
            jumped = parent[parent]
            if np.array_equal(jumped, parent):
                break
            parent = jumped
        if not changed:
            assert not parent.any() or n == 1          # one tree, rooted at the lowest index
            return rounds


def test_depth_of_a_sorted_chain_after_one_snapshot_round():
    """Hooked from a snapshot, a sorted chain is parent[i] = i - 1: depth n - 1, 14 pointer jumps at n = 2^14 -- more than the 8
    shortcut launches the round driver queues at a time."""
    n = SC.CHAIN_N
    for name in ("ascending", "descending"):
        index_of = SC.chain_order(name, n)
        a, b = index_of[:-1], index_of[1:]
        parent = np.arange(n, dtype=i64)
        np.minimum.at(parent, np.maximum(a, b), np.minimum(a, b))
        assert np.array_equal(parent, np.maximum(np.arange(n) - 1, 0))
        jumps = 0
        while parent.any():
            parent = parent[parent]
            jumps += 1
        assert jumps == 14 > 8


@pytest.mark.parametrize("n", [16, 256, 4096])
def test_hook_rounds_of_a_path_are_bounded_by_its_logarithm(n):
    """On a path the trees are contiguous runs, and a tree that is not the least among its neighbours loses its root in the
    round: of k trees at most ceil(k / 2) survive, so ceil(log2 n) rounds join them all and one more finds nothing to do.  The
    bit-reversed order attains the bound from a snapshot; no order or schedule tried exceeds it."""
    bound = math.ceil(math.log2(n)) + 1
    rng = np.random.default_rng([0x636C7573, 1, n])
    orders = {name: SC.chain_order(name, n) for name in SC.CHAIN_ORDERS}
    for s in range(3):
        orders[("shuffled", s)] = rng.permutation(n)
    assert hook_rounds(orders["bit_reversed"], "snapshot") == bound
    assert hook_rounds(orders["ascending"], "snapshot") == hook_rounds(orders["descending"], "snapshot") == 2
    for name, index_of in orders.items():
        for schedule in ("snapshot", "sequential", "random"):
            assert 2 <= hook_rounds(index_of, schedule, rng) <= bound, (name, schedule)
    assert bound == {16: 5, 256: 9, 4096: 13}[n] and math.ceil(math.log2(SC.CHAIN_N)) + 1 == 15


# ---- 2. the star -----------------------------------------------------------------------------------------------------------------
def test_star_layouts_have_what_they_are_there_for():
    assert len(SC.STAR_PERMUTATIONS) >= 6 and {p[0] for p in SC.STAR_PERMUTATIONS} == set(range(6))      # every direction wins once
    assert all(sorted(p) == list(range(6)) for p in SC.STAR_PERMUTATIONS)
    assert len(SC.STAR_LAYOUTS) == len(SC.STAR_PERMUTATIONS) * 3 * 4
    apart = 0
    for lay in SC.STAR_LAYOUTS:
        perm, where, frame = lay
        P, radius, centre, inner = SC.star(*lay)
        scale, offset = SC.STAR_FRAMES[frame]
        order = SC.STAR_PERMUTATIONS[perm]
        assert len(P) == 97 and radius == scale and centre == {"first": 0, "middle": 48, "last": 96}[where]
        assert np.array_equal(P[centre], np.array(offset, f32))
        # exact in binary32: the positions (points_cluster_stress_cases._exact), the differences from the centre and their squares
        rel = P.astype(f64) - np.array(offset, f64)
        assert np.array_equal((P - P[centre]).astype(f64), rel)
        d2 = KM._d2(P, P[centre][None])[0]
        assert np.array_equal(d2.astype(f64), (rel * rel).sum(axis=1))
        assert np.array_equal(d2[inner], np.full(6, f32(scale) * f32(scale))) and np.count_nonzero(d2 <= f32(scale) * f32(scale)) == 7
        for a in range(6):
            assert np.array_equal(rel[inner[a]], SC.STAR_DIRECTIONS[a] * scale)
        out = _model(("star",) + lay)
        assert out["stats"] == [6, 96, 1, 0] and sorted(out["sizes"]) == [16] * 5 + [17]
        assert out["counts"][centre] == 7 and not out["core"][centre] and set(np.delete(out["counts"], centre)) == {16, 17}
        assert list(out["labels"][inner]) == list(range(6))                     # cluster a is arm a, whatever the order of the inner points
        outer = np.setdiff1d(np.arange(97), np.append(inner, centre))
        assert inner.min() > outer.max() and list(out["labels"][outer]) == [a for a in range(6) for _ in range(15)]      # the inner points come after all outer ones
        # the centre follows the inner point of the lowest index ...
        low, high = int(inner.argmin()), int(inner.argmax())
        assert low == order[0] and high == order[5] and out["labels"][centre] == low
        # ... which is neither the lowest cluster number nor the cluster of the highest inner index
        apart += low not in (0, high)
    assert apart >= len(SC.STAR_LAYOUTS) // 2
    perm, where, frame = STAR_NAMED
    assert SC.STAR_PERMUTATIONS[perm][0] == 3 and SC.STAR_PERMUTATIONS[perm][5] == 0


# ---- 3. the waves ----------------------------------------------------------------------------------------------------------------
def test_waves_have_the_stated_pattern():
    P, border = SC.waves()
    out = _model("waves")
    assert len(P) == SC.WAVES_N == 485 == 7 * 64 + 37
    assert np.array_equal(out["labels"], SC.WAVES_LABELS) and np.array_equal(~out["core"] & (out["labels"] >= 0), border)
    assert out["stats"] == [4, 485 - 97 - 4, 4, 97] and list(out["sizes"]) == [191, 95, 65, 37]
    lab = [out["labels"][64 * w:64 * w + 64] for w in range(8)]
    core = [out["core"][64 * w:64 * w + 64] for w in range(8)]
    assert (lab[0] == 0).all() and core[0].all()
    assert lab[1][0] == -1 and (lab[1][1:] == 0).all()
    assert (lab[2][0::2] == 0).all() and (lab[2][1::2] == -1).all()
    assert (lab[3] == -1).all()
    assert (lab[4][:32] == 0).all() and (lab[4][32:] == 1).all()
    assert (lab[5][:63] == 1).all() and lab[5][63] == 2 and core[5].all()
    assert (lab[6] == 2).all() and list(np.flatnonzero(~core[6])) == list(SC.WAVES_BORDER_LANES)     # border lanes in a uniform wave
    assert len(lab[7]) == 37 and (lab[7] == 3).all()
    # every border point reaches one core point, at d2 = 1 exactly; the first of them has a nearer neighbour that is noise
    off, idx = CM.neighbours(P, SC.WAVES_RADIUS)
    first = 6 * 64 + SC.WAVES_BORDER_LANES[0]
    for i in np.flatnonzero(border):
        row = idx[off[i]:off[i + 1]]
        assert row[0] == i and row[-1] == 383 and out["core"][row].sum() == 1 and len(row) == (3 if i == first else 2)
    mid = idx[off[first] + 1]
    assert out["labels"][mid] == -1 and not out["core"][mid] and out["counts"][mid] == 2


# ---- 5. the pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.PAIRS_MODEL_N)
def test_pairs_in_closed_form_are_the_models(n):
    P = SC.pairs(n)
    rows = SC.pairs_rows(n)
    assert _same_rows(rows, CM.neighbours(P, SC.PAIRS_RADIUS))
    for mp in (1, 2, 3):
        out = CM.cluster(P, SC.PAIRS_RADIUS, mp, rows)
        assert _same(out, SC.pairs_expected(n, mp)), (n, mp)
    want = SC.pairs_expected(n, 1)
    assert want["n_clusters"] == (n + 1) // 2 and np.array_equal(want["labels"], np.arange(n) // 2)
    keep = SC.pairs_keep(want["n_clusters"])
    assert np.array_equal(CM.select(want["labels"], keep), SC.pairs_kept(n))


def test_the_large_pairs_cloud_crosses_the_scan_carry():
    cKDTree = pytest.importorskip("scipy.spatial").cKDTree
    n = SC.PAIRS_LARGE_N
    P = SC.pairs(n)
    assert n == 524_290 and -(-n // 2048) == 257 > 256                          # one block total beyond what one pass of k_scan_sums takes
    # all distances are 0.25 or 1 at the least: binary64 decides as binary32 does
    got = cKDTree(P.astype(f64)).query_pairs(0.5, output_type="ndarray")
    assert np.array_equal(got[np.argsort(got[:, 0])], np.arange(n).reshape(-1, 2))
    assert len(cKDTree(P.astype(f64)).query_pairs(0.99, output_type="ndarray")) == n // 2
    rows = SC.pairs_rows(n)
    assert np.array_equal(np.diff(rows[0]), np.full(n, 2)) and np.array_equal(rows[1].reshape(-1, 2)[:, 0], np.arange(n))
    for mp in (1, 2, 3):
        assert _same(CM.cluster(P, SC.PAIRS_RADIUS, mp, rows), SC.pairs_expected(n, mp)), mp
    want = SC.pairs_expected(n, 1)
    assert want["n_clusters"] == 262_145 and want["labels"][-1] == 262_144 and SC.pairs_expected(n, 3)["stats"] == [0, 0, 0, n]
    kept = SC.pairs_kept(n)
    assert np.array_equal(CM.select(want["labels"], SC.pairs_keep(want["n_clusters"])), kept)
    assert len(kept) > 256 * 2048 // 2 and kept[-1] == n - 3                    # kept on both sides of the carry of the select scan too


# ---- 6. overflow and underflow ---------------------------------------------------------------------------------------------------
def test_overflow_clumps_are_no_neighbours_at_any_radius():
    P, clump = SC.overflow()
    assert np.all(np.isfinite(P)) and sorted(np.bincount(clump)) == [40, 40]
    d2 = KM._d2(P, P)
    across = clump[:, None] != clump[None, :]
    assert np.all(np.isinf(d2[across])) and d2[~across].max() < 3e36
    for radius, mp, stats in SC.OVERFLOW_CASES:
        out = _model(("overflow", radius, mp))
        assert out["stats"] == stats
        if mp == 1:
            assert list(out["sizes"]) == [40, 40] and np.array_equal(out["labels"], (clump != clump[0]).astype(i32))
            assert (out["counts"] == 40).all()
    assert f32(3e38) < np.finfo(f32).max and not np.any(np.diff(np.sort(clump)) < 0) and np.any(np.diff(clump) < 0)      # shuffled


def test_underflow_makes_distinct_points_duplicates():
    P, tiny = SC.underflow()
    assert len(np.unique(P, axis=0)) == 100 and tiny.sum() == 50                # pairwise distinct
    assert np.all(P[tiny] != 0) and np.all(np.abs(P[tiny]) >= np.finfo(f32).tiny)      # (ordinary float32 numbers; only d2 underflows)
    d2 = KM._d2(P, P)
    assert not d2[np.ix_(tiny, tiny)].any()                                     # every d2 among the tiny ones is 0
    other = d2[~tiny]
    other[np.arange(50), np.flatnonzero(~tiny)] = 1                             # (but for a point's d2 to itself)
    assert np.all(other >= 1e-40)                                               # every other d2 is far from underflow
    for radius, mp, stats in SC.UNDERFLOW_CASES:
        out = _model(("underflow", radius, mp))
        assert out["stats"] == stats and sorted(out["sizes"]) == [1] * 50 + [50]
        assert len(set(out["labels"][tiny])) == 1 and (out["counts"][tiny] == 50).all() and (out["counts"][~tiny] == 1).all()
    assert f32(1e-45) > 0


# ---- the wrong variants ----------------------------------------------------------------------------------------------------------
def _rows_d2(P, radius, strict=False, accept_inf=False, binary64=False):
    """The neighbour rows with their d2, row by row: -> (offsets, index, d2).  As the model: d2 in binary32 by the contract's
    formula, +inf does not count, within iff the binary32 root is <= radius, ordered by (d2, index)."""
    P = np.asarray(P, f32)
    r = f32(radius)
    if binary64:
        Q = P.astype(f64)
        d2 = ((Q[:, None, :] - Q[None, :, :]) ** 2).sum(axis=2)
        root = np.sqrt(d2)
    else:
        d2 = KM._d2(P, P)
        root = KM._dist(d2)
    mask = (root < r) if strict else (root <= r)
    if not accept_inf:
        mask &= d2 < INF
    off, idx, val = [0], [], []
    for row, m in zip(d2, mask):
        j = np.flatnonzero(m)
        j = j[np.argsort(row[j], kind="stable")]
        off.append(off[-1] + len(j))
        idx.append(j)
        val.append(row[j])
    return np.array(off, i64), np.concatenate(idx).astype(i32), np.concatenate(val)


def _numbers(root, core, block=None):
    """-> (the ascending roots, every core point's cluster number).  block: the numbers restart at every multiple of it -- the
    scan of the root flags with the carry between two passes over the block totals dropped."""
    roots = np.unique(root[core])
    number = np.searchsorted(roots, root[core])
    if block is not None:
        number = number - np.searchsorted(roots, root[core] // block * block)
    return roots, number


def _cluster_with(P, radius, min_points, rows=None, *, count_self=True, one_round=False, tie=None, nearest_any=False, number_all=False,
                  sizes_core_only=False):
    """tests/points_cluster_model.cluster line by line over (offsets, index, d2) rows, with the places the wrong variants change."""
    off, idx, d2 = rows if rows is not None else _rows_d2(P, radius)
    n = len(P)
    per = np.diff(off)
    counts = (per if count_self else per - 1).astype(i32)
    core = counts >= int(min_points)
    src = np.repeat(np.arange(n, dtype=i64), per)
    dst = idx.astype(i64)
    edge = core[src] & core[dst]
    if one_round:
        root = np.arange(n, dtype=i64)
        pa, pb = src[edge], dst[edge]
        np.minimum.at(root, np.maximum(pa, pb), np.minimum(pa, pb))
        while not np.array_equal(root[root], root):
            root = root[root]
    else:
        root = CM.components(n, src[edge], dst[edge])
    roots, number = _numbers(root, core)
    labels = np.full(n, -1, i32)
    labels[core] = number
    for i in np.flatnonzero(~core):
        row, rd2 = dst[off[i]:off[i + 1]], d2[off[i]:off[i + 1]]
        if nearest_any:
            row = row[row != i]
            if len(row) and core[row[0]]:
                labels[i] = labels[row[0]]
            continue
        cand = np.flatnonzero(core[row])
        if not len(cand):
            continue
        ties = row[cand[rd2[cand] == rd2[cand[0]]]]                             # the core candidates at the least d2, by ascending index
        pick = ties[0] if tie is None else ties[-1] if tie == "higher_index" else ties[np.argmin(labels[ties])]
        labels[i] = labels[pick]
    if number_all and len(roots):
        lowest = np.full(len(roots), n, i64)
        np.minimum.at(lowest, labels[labels >= 0], np.flatnonzero(labels >= 0))
        rank = np.empty(len(roots), i64)
        rank[np.argsort(lowest)] = np.arange(len(roots))
        labels[labels >= 0] = rank[labels[labels >= 0]]
    members = labels[core] if sizes_core_only else labels[labels >= 0]
    sizes = np.bincount(members, minlength=len(roots)).astype(i32)
    border = ~core & (labels >= 0)
    return {"labels": labels, "sizes": sizes, "core": core, "counts": counts, "n_clusters": len(roots),
            "stats": [len(roots), int(core.sum()), int(border.sum()), int((labels < 0).sum())]}


def _differs_on(names=None, rows_with=None, **wrong):
    """The named cases on which the variant's result is not the model's."""
    hit = []
    for name in (names or _cases()):
        P, radius, mp = _cases()[name]
        rows = None if rows_with is None else _rows_d2(P, radius, **rows_with)
        if not _same(_cluster_with(P, radius, mp, rows, **wrong), _model(name)):
            hit.append(name)
    return hit


def _small_cases():
    """Every named case but most of the star's layouts (one per arm order, centre and frame is enough for the variants)."""
    return [n for n in _cases() if not (isinstance(n, tuple) and n[0] == "star") or n[2] == "first" or n[1:] == (1, "last", 3)]


def test_the_unchanged_lines_give_the_model():
    assert _differs_on(_small_cases()) == []
    for name in _small_cases():
        P, radius, _ = _cases()[name]
        assert _same_rows(_rows_d2(P, radius)[:2], CM.neighbours(P, radius)), name


def test_variant_1_a_border_tie_goes_to_the_lower_cluster_number():
    hit = _differs_on(_small_cases(), tie="lower_cluster")
    assert ("star",) + STAR_NAMED in hit and all(n[0] == "star" for n in hit)
    assert {SC.STAR_PERMUTATIONS[n[1]][0] for n in hit} == {1, 2, 3, 4, 5}       # wherever arm 0 does not win anyway


def test_variant_2_a_border_tie_goes_to_the_higher_index():
    hit = _differs_on(_small_cases(), tie="higher_index")
    assert ("star",) + STAR_NAMED in hit and ("star", 1, "last", 3) in hit and all(n[0] == "star" for n in hit)
    assert len(hit) == len([n for n in _small_cases() if n[0] == "star"])


def test_variant_3_a_border_point_takes_the_nearest_point_core_or_not():
    hit = _differs_on(_small_cases(), nearest_any=True)
    assert hit == ["waves"]


def test_variant_4_within_is_strict():
    hit = _differs_on(_small_cases(), rows_with={"strict": True})
    assert ("star",) + STAR_NAMED in hit and ("star", 1, "last", 3) in hit and "waves" in hit
    assert all(("chain", name, mp) in hit for name in SC.CHAIN_ORDERS for mp in (1, 3))
    assert ("underflow", 0.0, 1) in hit and ("pairs", 257) not in hit


def test_variant_5_radius_infinity_accepts_an_infinite_d2():
    hit = _differs_on(_small_cases(), rows_with={"accept_inf": True})
    assert hit == [("overflow", INF, 1), ("overflow", INF, 41)]                  # (3e38 is below +inf: not there)


def test_variant_6_clusters_numbered_by_their_lowest_member_border_included():
    hit = _differs_on(_small_cases(), number_all=True)
    assert ("star",) + STAR_NAMED in hit and all(n[0] == "star" and n[2] == "first" for n in hit)
    assert {SC.STAR_PERMUTATIONS[n[1]][0] for n in hit} == {1, 2, 3, 4, 5}


def test_variant_7_the_count_leaves_the_point_itself_out():
    hit = _differs_on(_small_cases(), count_self=False)
    assert set(hit) == set(_small_cases())
    P, radius, mp = _cases()[("chain", "bit_reversed", 3)]
    assert _cluster_with(P, radius, mp, count_self=False)["stats"] == [0, 0, 0, 1024]     # nothing is core any more
    P, radius, mp = _cases()["waves"]
    assert _cluster_with(P, radius, mp, count_self=False)["stats"][:2] == _model("waves")["stats"][:2]     # (there only the counts differ)


def test_variant_8_sizes_count_core_points_only():
    hit = _differs_on(_small_cases(), sizes_core_only=True)
    assert ("star",) + STAR_NAMED in hit and "waves" in hit and all(("chain", name, 3) in hit for name in SC.CHAIN_ORDERS)
    assert all(_model(n)["stats"][2] > 0 for n in hit)


def test_variant_9_labels_from_a_single_hook_round():
    hit = _differs_on(_small_cases(), one_round=True)
    assert ("chain", "bit_reversed", 1) in hit and ("chain", "bit_reversed", 3) in hit
    assert ("chain", "ascending", 1) not in hit and ("chain", "descending", 1) not in hit     # (one round and a deep flattening: the depth is their point)
    P, radius, mp = _cases()[("chain", "bit_reversed", 1)]
    assert _cluster_with(P, radius, mp, one_round=True)["n_clusters"] > 100


def test_variant_10_root_numbers_with_a_dropped_scan_carry():
    block = 256 * 2048
    for n in (4097, SC.PAIRS_LARGE_N):
        i = np.arange(n, dtype=i64)
        core = np.ones(n, bool)
        root = i - i % 2
        want = SC.pairs_expected(n, 1)["labels"]
        assert np.array_equal(_numbers(root, core)[1], want)
        dropped = _numbers(root, core, block)[1]
        if n <= block:
            assert np.array_equal(dropped, want)                                  # nothing below the large cloud shows it
        else:
            assert list(np.flatnonzero(dropped != want)) == [n - 2, n - 1] and list(dropped[-2:]) == [0, 0]
    # ... and the same in the scan of select's keep flags, under the opposite keep bytes (pairs_keep drops the last cluster, whose two
    # points are all of the last scan block): the kept ones of the last block land on those of the first
    n = SC.PAIRS_LARGE_N
    labels = SC.pairs_expected(n, 1)["labels"]
    assert not SC.pairs_keep(262_145)[-1]
    keep = (1 - SC.pairs_keep(262_145))[labels].astype(i64)
    slot = np.cumsum(keep) - keep
    dropped = slot - slot[np.arange(n) // block * block]
    kept = np.flatnonzero(keep)
    assert np.array_equal(kept, CM.select(labels, 1 - SC.pairs_keep(262_145))) and list(kept[-2:]) == [n - 2, n - 1]
    assert np.array_equal(slot[kept], np.arange(len(kept))) and list(dropped[kept][-2:]) == [0, 1] == list(dropped[kept][:2])


def test_variant_11_select_keeps_a_label_equal_to_n_clusters():
    def wrong(labels, keep):
        keep = np.concatenate([np.asarray(keep, bool), [True]])                   # (what lies behind the keep bytes)
        labels = np.asarray(labels)
        ok = (labels >= 0) & (labels <= len(keep) - 1)
        ok[ok] = keep[labels[ok]]
        return np.flatnonzero(ok).astype(i32)
    labels = _model(("pairs", 257))["labels"]
    full = SC.pairs_keep(129)
    assert np.array_equal(wrong(labels, full), CM.select(labels, full))            # no label reaches n_clusters: the named case below does
    short = np.ones(128, np.uint8)                                                # the keep bytes of all clusters but the last
    assert list(CM.select(labels, short)) == list(range(256)) and list(wrong(labels, short)) == list(range(257))


def test_variant_12_d2_in_binary64():
    hit = _differs_on(_small_cases(), rows_with={"binary64": True})
    # (the overflow cloud shows it as well: in binary64 no d2 there is infinite)
    assert hit == [("overflow",) + c[:2] for c in SC.OVERFLOW_CASES] + [("underflow", 0.0, 1), ("underflow", 1e-45, 1)]
    P, radius, mp = _cases()[("underflow", 0.0, 1)]
    assert _cluster_with(P, radius, mp, _rows_d2(P, radius, binary64=True))["stats"] == [100, 100, 0, 0]
