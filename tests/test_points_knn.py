"""CPU checks of KdTree's k-nearest and radius queries: the numpy model (tests/points_knn_model.py) on hand-made cases and
against tests/points_model.nearest, the shared arithmetic of the kernels (sdfkit_amd/csrc/points_knn.h) built with g++ against
numpy, and the six new C-ABI entry points: exported, and refusing to run without a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from sdfkit_amd import _native as N
from tests import points_knn_model as KM
from tests import points_model as PM

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["sdfk_points_knn", "sdfk_points_knn_device", "sdfk_points_radius_count", "sdfk_points_radius_count_device",
                "sdfk_points_radius_fill", "sdfk_points_radius_fill_device"]
KEY_INF = np.uint64(0x7F800000) << np.uint64(32)


def _bits(x):
    return np.asarray(x, f32).view(np.uint32)


# ---- the model on hand-made cases ----
def test_model_ties_and_duplicates():
    P = np.array([[1, 0, 0], [0, 0, 0], [-1, 0, 0], [0, 0, 0], [0, 1, 0], [0, -1, 0]], f32)
    idx, dist, found = KM.knn(P, [[0, 0, 0]], 6)
    assert list(idx[0]) == [1, 3, 0, 2, 4, 5]           # the duplicates of the query first, then the four ties in index order
    assert list(dist[0]) == [0, 0, 1, 1, 1, 1] and found[0] == 6
    idx, _, _ = KM.knn(P, [[0, 0, 0]], 3)
    assert list(idx[0]) == [1, 3, 0]


def test_model_fewer_than_k_points():
    idx, dist, found = KM.knn(PM.THREE_POINTS, [[0.0, 1.5, 0.0]], 8)
    assert found[0] == 3 and idx[0, 0] == 1 and sorted(idx[0, :3]) == [0, 1, 2]
    assert (idx[0, 3:] == -1).all() and (dist[0, 3:] == KM.FLT_MAX).all()
    assert dist[0, 0] == f32(0.5)


def test_model_nonfinite_and_overflowing_queries():
    P = np.array([[0, 0, 0], [1, 0, 0]], f32)
    Q = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0], [3e38, 3e38, 3e38]], f32)
    idx, dist, found = KM.knn(P, Q, 2)
    assert (idx == -1).all() and (dist == KM.FLT_MAX).all() and (found == 0).all()
    off, ri, rd = KM.radius(P, Q, np.inf)
    assert (off == 0).all() and len(ri) == 0 and len(rd) == 0


def test_model_radius_at_a_distance_and_one_ulp_below():
    rs = np.random.default_rng(0)
    P = rs.random((200, 3), dtype=f32)
    q = rs.random((1, 3), dtype=f32)
    _, dist, _ = KM.knn(P, q, 64)
    for d in dist[0][[0, 5, 17, 63]]:
        below = np.nextafter(d, f32(0))
        n_at = int(KM.radius(P, q, d)[0][1])
        n_below = int(KM.radius(P, q, below)[0][1])
        assert n_at == int((dist[0] <= d).sum()) and n_below == int((dist[0] < d).sum()) and n_below < n_at
        _, _, f_at = KM.knn(P, q, 64, d)
        _, _, f_below = KM.knn(P, q, 64, below)
        assert f_at[0] == n_at and f_below[0] == n_below


def test_model_radius_zero_and_infinite():
    P = np.array([[0.5, 0.25, 2], [1, 1, 1], [0.5, 0.25, 2], [3, 3, 3]], f32)
    off, idx, dist = KM.radius(P, [[0.5, 0.25, 2], [1, 1, 1.5]], 0.0)
    assert list(off) == [0, 2, 2] and list(idx) == [0, 2] and list(dist) == [0, 0]
    off, idx, dist = KM.radius(P, [[1, 1, 1.5]], np.inf)
    assert list(off) == [0, 4] and list(idx) == [1, 0, 2, 3]
    assert np.array_equal(_bits(dist), _bits(KM.knn(P, [[1, 1, 1.5]], 4)[1][0]))


def _tie_heavy(rs, n, m):
    P = rs.integers(0, 4, (n, 3)).astype(f32)
    Q = (rs.integers(0, 8, (m, 3)) * 0.5).astype(f32)
    return P, Q


def test_model_k1_equals_nearest():
    rs = np.random.default_rng(1)
    cases = [(rs.random((3000, 3), dtype=f32), rs.random((500, 3), dtype=f32)), _tie_heavy(rs, 400, 300)]
    cases.append((cases[0][0], np.array([[np.nan, 0, 0], [1e30, 0, 0], [3e38, -3e38, 0]], f32)))
    for P, Q in cases:
        idx, dist, found = KM.knn(P, Q, 1)
        ri, rd, _ = PM.nearest(P, Q)
        assert np.array_equal(idx[:, 0], ri) and np.array_equal(_bits(dist[:, 0]), _bits(rd))
        assert np.array_equal(found, (ri >= 0).astype(np.int32))


def test_model_radius_prefix_equals_knn():
    rs = np.random.default_rng(2)
    for P, Q, r in [(rs.random((2000, 3), dtype=f32), rs.random((100, 3), dtype=f32), 0.2), _tie_heavy(rs, 300, 100) + (1.5,)]:
        off, ri, rd = KM.radius(P, Q, r)
        for k in (1, 5, 64):
            idx, dist, found = KM.knn(P, Q, k, r)
            for i in range(len(Q)):
                n = min(k, int(off[i + 1] - off[i]))
                assert found[i] == n
                assert np.array_equal(idx[i, :n], ri[off[i]:off[i] + n]) and np.array_equal(_bits(dist[i, :n]), _bits(rd[off[i]:off[i] + n]))
                assert (idx[i, n:] == -1).all() and (dist[i, n:] == KM.FLT_MAX).all()


# ---- the kernels' arithmetic, built for the host ----
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("points_knn_host")
    exe = str(d / "points_knn_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "points_knn_host.cpp"), "-o", exe])

    def run(mode, data, out_dtype):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        data.tofile(fin)
        p = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and f"points_knn_host {mode} ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
        return np.fromfile(fout, out_dtype)
    return run


def _keys(rs, m, mass_ties):
    """m packed keys, some at or above kKeyInf (not counting); mass_ties: a handful of d2 values only."""
    if mass_ties:
        d2 = rs.choice(np.array([0.0, 0.25, 0.25, 1.0, 2.5, np.inf], f32), m)
    else:
        d2 = (rs.random(m, dtype=f32) * f32(10)) ** 2
        d2[rs.random(m) < 0.05] = np.inf
    index = rs.permutation(max(m, 1))[:m].astype(np.uint64)       # (an insertion index occurs once)
    return (_bits(d2).astype(np.uint64) << np.uint64(32)) | index


def test_host_bounded_lists_equal_sorted_prefix(host):
    rs = np.random.default_rng(3)
    cases = 0
    for kind, ks in ((0, (1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64)), (1, (1, 2, 3, 7, 8))):
        for k in ks:
            for m in (0, 1, k - 1, k, k + 1, 5 * k + 3, 2000):
                for mass_ties in (False, True):
                    keys = _keys(rs, m, mass_ties)
                    out = host("list", np.concatenate([np.array([kind, k, m], np.uint64), keys]), np.uint64)
                    want = np.sort(keys[keys < KEY_INF])[:k]
                    assert out[0] == len(want), (kind, k, m, mass_ties)
                    assert np.array_equal(out[1:1 + len(want)], want), (kind, k, m, mass_ties)
                    assert (out[1 + len(want):] == KEY_INF).all() and len(out) == 1 + k
                    cases += 1
    assert cases == 16 * 7 * 2


def test_host_heap_sort_orders_segments(host):
    rs = np.random.default_rng(4)
    for m in (0, 1, 2, 3, 10, 257, 5000):
        for mass_ties in (False, True):
            keys = _keys(rs, m, mass_ties)
            out = host("sort", np.concatenate([np.array([m], np.uint64), keys]), np.uint64)
            assert np.array_equal(out, np.sort(keys))


def test_host_radius_predicate_at_the_neighbours_of_thresholds(host):
    """within(d2, radius_d2_bound(r)) == (sqrtf(d2) <= r) for the d2 values around r * r, for many r of every size."""
    rs = np.random.default_rng(5)
    r = np.concatenate([np.exp(rs.uniform(np.log(1e-30), np.log(1e25), 4000)).astype(f32), rs.random(2000, dtype=f32),
                        np.array([0.0, 1e-45, 1e-39, 1.1754944e-38, 1.0, 2.0, 3.0, 1.8446743e19, 1.8446744e19, 3e38, KM.FLT_MAX, np.inf], f32)])
    with np.errstate(over="ignore"):
        centre = (r.astype(np.float64) ** 2).astype(f32)
    centre = np.minimum(centre, KM.FLT_MAX).view(np.uint32).astype(np.int64)
    pairs = []
    for delta in range(-4, 5):
        d2 = np.clip(centre + delta, 0, 0x7F800000).astype(np.uint32)   # (up to +inf, never NaN or negative)
        pairs.append(np.stack([r.view(np.uint32), d2], axis=1))
    pairs = np.concatenate(pairs)
    out = host("radius", np.concatenate([np.array([len(pairs)], np.uint32), pairs.reshape(-1)]), np.uint32).reshape(-1, 2)
    rr, d2 = pairs[:, 0].copy().view(f32), pairs[:, 1].copy().view(f32)
    dist = np.sqrt(d2.astype(np.float64)).astype(f32)
    want = (d2 < np.inf) & (dist <= rr)
    assert np.array_equal(out[:, 1], want.astype(np.uint32))
    assert want.any() and (~want).any()
    # the bound itself: the largest finite d2 whose root is <= r
    b = out[:, 0].copy().view(f32)
    assert (np.sqrt(b.astype(np.float64)).astype(f32) <= rr).all() and (b <= KM.FLT_MAX).all()
    with np.errstate(over="ignore"):
        up = np.nextafter(b, f32(np.inf))
    assert ((up == np.inf) | (np.sqrt(up.astype(np.float64)).astype(f32) > rr)).all()
    # refused radii
    bad = np.array([[_bits(f32(-1.0)), 0], [_bits(f32(np.nan)), 0], [_bits(f32(-0.0)), 0]], np.uint32)
    out = host("radius", np.concatenate([np.array([3], np.uint32), bad.reshape(-1)]), np.uint32).reshape(-1, 2)
    assert list(out[:, 1]) == [2, 2, 1]   # (-0 is 0)


def test_host_stopping_rule(host):
    """walk_done(lb2, worst, bound) == lb2 * (1 - 2^-18) > min(d2 of worst, bound), in float32."""
    rs = np.random.default_rng(6)
    m = 5000
    lb2 = (rs.random(m, dtype=f32) * f32(4)).astype(f32)
    worst = np.where(rs.random(m) < 0.3, f32(np.inf), rs.random(m, dtype=f32) * f32(4)).astype(f32)
    bound = np.where(rs.random(m) < 0.3, KM.FLT_MAX, rs.random(m, dtype=f32) * f32(4)).astype(f32)
    lb2[:200] = worst[:200]                         # the strict inequality and the margin
    with np.errstate(over="ignore"):
        lb2[200:400] = np.nextafter(bound[200:400], f32(np.inf))
    lb2[400:410] = np.inf
    trip = np.stack([_bits(lb2), _bits(worst), _bits(bound)], axis=1)
    out = host("stop", np.concatenate([np.array([m], np.uint32), trip.reshape(-1)]), np.uint32)
    want = (lb2 * (f32(1) - f32(2.0 ** -18))) > np.minimum(worst, bound)
    assert np.array_equal(out, want.astype(np.uint32))
    assert not out[:200][worst[:200] <= bound[:200]].any()   # (lb2 == the worst d2: a tie may still be out there)


# ---- the C ABI ----
def test_points_knn_entry_points_exported():
    L = N.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in N.SIGNATURES, name


def test_points_knn_refuse_without_device():
    """No device (or sdfk_init not called): every new compute entry point returns SDFK_ERR_NO_DEVICE, in a fresh process."""
    p = subprocess.run([sys.executable, "-c", "from tests.test_points_knn import _refusals; _refusals(); print('refusals ok')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "refusals ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def _refusals():
    L = N.lib()
    pts = np.zeros((3, 3), f32)
    P = C.c_void_p(pts.ctypes.data)
    off = np.zeros(4, np.int64)
    O = C.c_void_p(off.ctypes.data)
    calls = {
        "sdfk_points_knn": lambda: L.sdfk_points_knn(None, P, 3, 1, np.inf, None, None, None),
        "sdfk_points_knn_device": lambda: L.sdfk_points_knn_device(None, P, 3, 1, np.inf, None, None, None),
        "sdfk_points_radius_count": lambda: L.sdfk_points_radius_count(None, P, 3, 1.0, O),
        "sdfk_points_radius_count_device": lambda: L.sdfk_points_radius_count_device(None, P, 3, 1.0, O),
        "sdfk_points_radius_fill": lambda: L.sdfk_points_radius_fill(None, P, 3, 1.0, O, None, None),
        "sdfk_points_radius_fill_device": lambda: L.sdfk_points_radius_fill_device(None, P, 3, 1.0, O, None, None),
    }
    assert sorted(calls) == sorted(ENTRY_POINTS)
    for name, call in calls.items():
        assert call() == N.ERR_NO_DEVICE, name
