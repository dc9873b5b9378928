"""CPU checks of the KdTree's density clustering: the numpy model (tests/points_cluster_model.py) against a restatement in plain
loops, against scikit-learn's DBSCAN where it is installed (core set, noise set, the partition of the core points; not the border
labels, which are order-dependent there) and against the recorded counts of tests/golden/points_cluster_cases.json; the decisions
of the kernels (sdfkit_amd/csrc/points_cluster.h) built with g++ against the model, argument for argument; and the four new C-ABI
entry points: exported, refusing to run without a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from sdfkit_amd import _native as N
from tests import points_cluster_cases as CC
from tests import points_cluster_model as CM
from tests import points_knn_model as KM

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["sdfk_points_cluster", "sdfk_points_cluster_device", "sdfk_points_select", "sdfk_points_select_device"]
GOLD = CC.golden()


def slow_cluster(P, radius, min_points):
    """The contract in plain Python loops: the predicate pair by pair, union-find over the core pairs, the border by a scan for the
    least (d2, index)."""
    P = np.asarray(P, f32).reshape(-1, 3)
    n = len(P)
    r = f32(radius)
    d2 = np.full((n, n), np.inf, f32)
    within = np.zeros((n, n), bool)
    for i in range(n):
        for j in range(n):
            dx, dy, dz = P[i, 0] - P[j, 0], P[i, 1] - P[j, 1], P[i, 2] - P[j, 2]
            d = f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz)
            if d < np.inf:
                d2[i, j] = d
                within[i, j] = f32(np.sqrt(np.float64(d))) <= r
    counts = within.sum(axis=1)
    core = counts >= min_points
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for i in range(n):
        for j in range(n):
            if core[i] and core[j] and within[i, j]:
                a, b = find(i), find(j)
                parent[max(a, b)] = min(a, b)
    labels = np.full(n, -1, np.int32)
    number = {}
    for i in range(n):               # ascending: a cluster is met first at its lowest core member
        if core[i]:
            labels[i] = number.setdefault(find(i), len(number))
    for i in range(n):
        if not core[i]:
            best = None
            for j in range(n):
                if core[j] and within[i, j] and (best is None or (d2[i, j], j) < best):
                    best = (d2[i, j], j)
            if best is not None:
                labels[i] = labels[best[1]]
    sizes = np.bincount(labels[labels >= 0], minlength=len(number)).astype(np.int32)
    return labels, sizes, core, counts.astype(np.int32)


def same(out, slow):
    return all(np.array_equal(out[k], s) for k, s in zip(("labels", "sizes", "core", "counts"), slow))


# ---- the model ----
def test_model_against_the_plain_loops_on_a_random_cloud():
    rs = np.random.default_rng(3)
    P = np.concatenate([rs.standard_normal((150, 3)) * 0.5, rs.standard_normal((100, 3)) * 0.3 + 2.5, rs.uniform(-4, 4, (30, 3))]).astype(f32)
    P[40:50] = P[:10]                                  # duplicates
    seen = set()
    for radius, mp in ((0.3, 1), (0.3, 4), (0.45, 8), (0.0, 2), (np.inf, 1), (0.2, 3)):
        out = CM.cluster(P, radius, mp)
        assert same(out, slow_cluster(P, radius, mp)), (radius, mp)
        seen.add((out["stats"][2] > 0, out["stats"][3] > 0))
    assert (True, True) in seen                        # a border and noise were there to get wrong


def test_model_on_the_tie_in_its_three_orders():
    for name, P, labels, sizes in CC.tie_clouds():
        out = CM.cluster(P, 1.0, 4)
        assert list(out["labels"]) == labels and list(out["sizes"]) == sizes == [5, 4], name
        assert same(out, slow_cluster(P, 1.0, 4))
        origin = int(np.flatnonzero((P == 0).all(axis=1))[0])
        assert out["counts"][origin] == 3 and not out["core"][origin]
        # at exactly distance 1 from one core point of either side, and the lower index wins
        row = np.flatnonzero(np.sqrt(((P - P[origin]) ** 2).sum(axis=1)) == 1.0)
        assert len(row) == 2 and out["labels"][origin] == out["labels"][row.min()] != out["labels"][row.max()]
    assert [t[2] for t in CC.tie_clouds()] == [[0, 0, 0, 0, 1, 1, 1, 1, 0], [0, 0, 0, 0, 1, 1, 1, 1, 0], [0, 0, 0, 0, 0, 1, 1, 1, 1]]


def test_model_reductions_and_refusals():
    P = CC.duplicates()
    out = CM.cluster(P, 0.0, 1)
    assert out["stats"] == [9, 19, 0, 0] and sorted(out["sizes"]) == [1] * 4 + [3] * 5          # radius 0: exact duplicates only
    assert CM.cluster(P, 0.0, 3)["stats"] == [5, 15, 0, 4] and CM.cluster(P, 0.0, 4)["stats"] == [0, 0, 0, 19]
    assert CM.cluster(P, np.inf, 1)["stats"] == [1, 19, 0, 0] and CM.cluster(P, np.inf, 20)["stats"] == [0, 0, 0, 19]
    out = CM.cluster(P, 0.4, 1)                                                                 # min_points = 1: all core, no noise
    assert out["core"].all() and (out["labels"] >= 0).all() and out["sizes"].sum() == len(P)
    for radius, mp in ((-1.0, 1), (np.nan, 1), (-np.inf, 1), (0.5, 0), (0.5, -1)):
        with pytest.raises(CM.Refused):
            CM.cluster(P, radius, mp)
    with pytest.raises(CM.Refused):
        CM.select([0, 1], [1], -1)
    assert list(CM.select([0, -1, 2, 1, 5, 1], [0, 1, 1])) == [2, 3, 5] and list(CM.select([0, 1], [])) == []
    assert CM.largest([3, 7, 7, 1]) == 1 and CM.largest([]) == -1


@pytest.mark.parametrize("radius,min_points", CC.A_CASES)
def test_cloud_a_numbers(radius, min_points):
    P, which = CC.cloud_a()
    out = CM.cluster(P, radius, min_points)
    rec = GOLD["cloud_a"][f"{radius},{min_points}"]
    sizes = sorted((int(s) for s in out["sizes"]), reverse=True)
    assert out["stats"] == rec["stats"] and sizes[:4] == rec["largest_sizes"] and sizes.count(1) == rec["singletons"]
    if (radius, min_points) == (0.2, 1):
        assert out["n_clusters"] == 43 and sizes[:3] == [1500, 700, 300] and sizes[3:] == [1] * 40
        big = np.argsort(-out["sizes"], kind="stable")[:3]
        for c, w in zip(big, (0, 1, 2)):
            assert (which[out["labels"] == c] == w).all()
    elif (radius, min_points) == (0.2, 6):
        assert out["stats"] == [3, 2500, 0, 40] and (out["labels"][which == 3] == -1).all()
    else:
        assert out["stats"] == [42, 938, 617, 985]


def test_recorded_counts_of_the_small_clouds():
    P = CC.chain()
    rows = CM.neighbours(P, 1.0)
    for name, radius, mp, r in (("1,1", 1.0, 1, rows), ("below_1,1", CC.BELOW_ONE, 1, None), ("1,3", 1.0, 3, rows)):
        assert CM.cluster(P, radius, mp, r)["stats"] == GOLD["chain"][name]["stats"]
    assert GOLD["chain"]["1,1"]["stats"] == [1, 4096, 0, 0] and GOLD["chain"]["below_1,1"]["stats"][0] == 4096 and GOLD["chain"]["1,3"]["stats"] == [1, 4094, 2, 0]
    F = CC.far_cloud()
    assert np.abs(np.diff(np.unique(F[:, 0]))).min() == 0.0625 and len(np.unique(F, axis=0)) < len(F)
    for radius, mp in ((0.25, 1), (0.5, 4)):
        assert CM.cluster(F, radius, mp)["stats"] == GOLD["far"][f"{radius},{mp}"]["stats"]
    assert GOLD["far"]["0.5,4"]["largest_sizes"] == [600]
    assert GOLD["two_sheets"]["0.1,1"]["largest_sizes"] == [10000, 10000] and GOLD["two_sheets"]["0.31,8"]["largest_sizes"] == [20000]
    assert GOLD["two_sheets"]["0.1,8"]["stats"][0] == 2 and 12 <= GOLD["two_sheets"]["0.1,8"]["stats"][2] <= 120


@pytest.mark.parametrize("radius,min_points", CC.A_CASES)
def test_model_against_scikit_learn(radius, min_points):
    cluster = pytest.importorskip("sklearn.cluster")
    P, _ = CC.cloud_a()
    out = CM.cluster(P, radius, min_points)
    # (float64 distances of the float32 points decide there, float32 ones here: three subtractions, three squares, two sums and a root
    # of binary32 err by less than 8 * 2^-24 of the distance, below 1e-7 at these radii, and no pair of this cloud is that close to one)
    D = np.sqrt(((P[:, None, :].astype(np.float64) - P[None, :, :].astype(np.float64)) ** 2).sum(axis=2))
    assert np.abs(D - np.float64(f32(radius))).min() > 2e-7
    db = cluster.DBSCAN(eps=float(f32(radius)), min_samples=min_points, algorithm="brute").fit(P.astype(np.float64))
    core = np.zeros(len(P), bool)
    core[db.core_sample_indices_] = True
    assert np.array_equal(core, out["core"]) and np.array_equal(db.labels_ < 0, out["labels"] < 0)
    pairs = set(zip(out["labels"][core].tolist(), db.labels_[core].tolist()))
    assert len(pairs) == out["n_clusters"] == len({a for a, _ in pairs}) == len({b for _, b in pairs})      # a bijection


# ---- points_cluster.h, built for the host ----
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("points_cluster_host")
    exe = str(d / "points_cluster_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "points_cluster_host.cpp"), "-o", exe])

    def run(mode, data):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        data.tofile(fin)
        p = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and f"points_cluster_host {mode} ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
        return np.fromfile(fout, np.int64)
    return run


def test_host_within_equals_the_radius_predicate(host):
    rs = np.random.default_rng(41)
    for r in (0.0, 0.12, 0.2, 1.0, CC.BELOW_ONE, 3e19, np.inf, 1e-30):
        r = f32(r)
        rr = f32(min(np.float64(r) ** 2, np.finfo(f32).max))
        near = rr.view(np.uint32).astype(np.int64) + np.arange(-40, 41)
        near = near[(near >= 0) & (near <= 0x7f800000)].astype(np.uint32).view(f32)
        with np.errstate(all="ignore"):
            d2 = np.concatenate([near, rs.random(50).astype(f32) * rr * 2, np.array([0.0, np.inf, np.nan, np.finfo(f32).max], f32)])
            want = (d2 < np.inf) & (np.sqrt(d2.astype(np.float64)).astype(f32) <= r)          # tests/points_knn_model.radius' mask
        got = host("within", np.concatenate([np.array([r], f32), d2]))
        assert np.array_equal(got.astype(bool), want), r
        assert want.any() and (not want.all())


def test_host_core_rule_equals_the_model(host):
    big = np.iinfo(np.int32).max
    pairs = np.array([(c, m) for c in (0, 1, 2, 5, 6, 9, 10, 11, big - 1, big) for m in (1, 2, 6, 10, big)], np.int32)
    out = host("core", pairs.reshape(-1)).reshape(-1, 2)
    assert np.array_equal(out[:, 0].astype(bool), pairs[:, 0] >= pairs[:, 1])
    assert np.array_equal(out[:, 1], np.minimum(pairs[:, 0].astype(np.int64) + 1, big))        # saturates
    P, _ = CC.cloud_a()
    m = CM.cluster(P[:600], 0.3, 5)
    out = host("core", np.stack([m["counts"], np.full(600, 5, np.int32)], axis=1).reshape(-1)).reshape(-1, 2)
    assert np.array_equal(out[:, 0].astype(bool), m["core"]) and 0 < m["core"].sum() < 600


def test_host_hook_target_equals_the_model(host):
    rs = np.random.default_rng(42)
    q = rs.integers(0, 12, (400, 4)).astype(np.int32)
    out = host("hook", q.reshape(-1)).reshape(-1, 6)
    pi, pj, old, i = (q[:, k].astype(np.int64) for k in range(4))
    hooked = pi != pj
    assert np.array_equal(out[:, 0].astype(bool), hooked) and hooked.any() and not hooked.all()
    assert np.array_equal(out[hooked, 1], np.maximum(pi, pj)[hooked]) and np.array_equal(out[hooked, 2], np.minimum(pi, pj)[hooked])
    assert np.array_equal(out[:, 3].astype(bool), hooked & (old > np.minimum(pi, pj)))           # "changed": the parent went down
    assert np.array_equal(out[:, 4].astype(bool), pi == i) and not out[:, 5].any()               # a point that is not core is no root
    # the rounds of the model end where no edge hooks: every core edge joins equal labels
    P, _ = CC.cloud_a()
    m = CM.cluster(P[:600], 0.3, 5)
    off, idx = CM.neighbours(P[:600], 0.3)
    src = np.repeat(np.arange(600), np.diff(off))
    e = m["core"][src] & m["core"][idx]
    quad = np.stack([m["labels"][src[e]], m["labels"][idx[e]], m["labels"][src[e]], src[e]], axis=1).astype(np.int32)
    assert not host("hook", quad.reshape(-1)).reshape(-1, 6)[:, 0].any() and len(quad) > 600


def _keys(d2, index):
    return np.asarray(d2, f32).view(np.uint32).astype(np.uint64) << np.uint64(32) | np.asarray(index, np.int64).astype(np.uint32).astype(np.uint64)


def test_host_border_choice_equals_the_model(host):
    P, _ = CC.cloud_a()
    cases = [(P[:900], 0.25, 6)] + [(t[1], 1.0, 4) for t in CC.tie_clouds()]
    flat, want = [], []
    for Q, radius, mp in cases:
        m = CM.cluster(Q, radius, mp)
        bound = int(_keys(f32(radius) * f32(radius), -1))   # (these radii square exactly enough: the bound is checked by `within` above)
        d2 = KM._d2(Q, Q)
        for i in np.flatnonzero(~m["core"]):
            cand = np.flatnonzero(d2[i] < np.float32(4 * radius * radius))      # candidates beyond the radius too, in index order
            cand = cand[::-1] if i % 2 else cand                                # ... and in the opposite order: the choice is a minimum
            keys = _keys(d2[i, cand], cand)
            flat += [bound, len(cand)] + [v for k, j in zip(keys.tolist(), cand) for v in (k, int(m["core"][j]))]
            inside = cand[(keys <= bound) & m["core"][cand]]
            src = int(inside[np.argmin(_keys(d2[i, inside], inside))]) if len(inside) else -1
            want.append(src)
            assert (m["labels"][i] == -1) if src < 0 else (m["labels"][i] == m["labels"][src])
    data = np.array([len(want)] + flat, np.uint64)
    assert np.array_equal(host("border", data), np.array(want, np.int64)) and min(want) == -1 and max(want) >= 0
    # nothing within the bound, and a key of exactly the bound
    data = np.array([2, 5 << 32 | 0xffffffff, 2, 6 << 32, 1, 5 << 32 | 7, 0, 5 << 32 | 0xffffffff, 1, 5 << 32 | 0xffffffff, 1], np.uint64)
    assert list(host("border", data)) == [-1, -1]           # (index 0xffffffff reads as -1: no static point has it)


def test_host_select_keep_rule_equals_the_model(host):
    rs = np.random.default_rng(43)
    labels = np.concatenate([rs.integers(-4, 12, 300), [np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, 0, 7, 8]]).astype(np.int64)
    for keep in ([1, 0, 1, 1, 0, 0, 1, 1], [0] * 8, [1] * 8, [1], []):
        got = host("select", np.concatenate([[len(keep)], keep, labels]).astype(np.int64))
        assert np.array_equal(np.flatnonzero(got), CM.select(labels, keep)), keep


def test_host_refusals_equal_the_model(host):
    P = CC.duplicates()
    radii = [0.0, -0.0, 1e-45, 0.5, 3e38, np.inf, -np.inf, np.nan, -1e-45, -1.0]
    rows, want = [], []
    for r in radii:
        for mp in (1, 2, 0, -1, np.iinfo(np.int32).min, np.iinfo(np.int32).max):
            rows.append([1, r, mp, 1, 1, 1, 3])
            try:
                CM.cluster(P, r, mp)
                want.append(0)
            except CM.Refused:
                want.append(2 if not (f32(r) >= 0) else 3)
    out = host("args", np.array(rows, np.float64).reshape(-1)).reshape(-1, 3)
    assert list(out[:, 0]) == want and 0 in want and 2 in want and 3 in want
    assert (out[:, 1] == 0).all() and (out[:, 2] == 4).all()
    # a NULL set comes first; select: set, labels, the count, then the keep bytes (not needed for no cluster)
    rows = [[0, np.nan, 0, 0, 0, 0, -1], [1, 1, 1, 1, 0, 0, -1], [1, 1, 1, 1, 1, 0, -1], [1, 1, 1, 1, 1, 0, 2], [1, 1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1, 0]]
    out = host("args", np.array(rows, np.float64).reshape(-1)).reshape(-1, 3)
    assert list(out[:, 0]) == [1, 0, 0, 0, 0, 0] and list(out[:, 1]) == [1, 4, 5, 6, 0, 0]


# ---- the C ABI ----
def test_cluster_entry_points_exported():
    L = N.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in N.SIGNATURES, name


def test_cluster_entry_points_refuse_without_device():
    """No device (or sdfk_init not called): the four entry points return SDFK_ERR_NO_DEVICE, outputs and stats untouched, in a
    fresh process."""
    p = subprocess.run([sys.executable, "-c", "from tests.test_points_cluster_model import _refusals; _refusals(); print('refusals ok')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "refusals ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def _refusals():
    L = N.lib()
    n = 5
    labels, sizes, core, counts = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, 7, np.uint8), np.full(n, -7, np.int32)
    idx, pts, keep = np.full(n, -7, np.int32), np.full((n, 3), -7, f32), np.ones(2, np.uint8)
    c = C.c_int64(-7)
    st = (C.c_int64 * 6)(*[-7] * 6)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for name in ENTRY_POINTS[:2]:
        for radius, mp in ((0.5, 1), (-1.0, 1), (float("nan"), 1), (0.5, 0)):      # bad arguments too: still nothing is touched
            assert getattr(L, name)(None, radius, mp, p(labels), p(sizes), p(core), p(counts), C.byref(c), st) == N.ERR_NO_DEVICE, name
    for name in ENTRY_POINTS[2:]:
        for nc in (2, -1):
            assert getattr(L, name)(None, p(labels), p(keep), nc, p(idx), p(pts), C.byref(c)) == N.ERR_NO_DEVICE, name
    assert (labels == -7).all() and (sizes == -7).all() and (core == 7).all() and (counts == -7).all() and (idx == -7).all() and (pts == -7).all()
    assert c.value == -7 and list(st) == [-7] * 6
