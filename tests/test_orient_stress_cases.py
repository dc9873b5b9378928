"""CPU proof that the clouds of tests/orient_stress_cases.py have the properties the device tests (tests/test_gpu_orient_stress.py)
rely on, by the numpy model (tests/orient_model.py) alone: the seeds of the long lines and the trip of the seed search they fall
into, the closed-form rows against the brute force, the rounds of the ladders against the batch length of the source, a link
accepted at every level and the zeros that keep their normal, the tie of two sources, the small edges, the seeds at max_distance = 0.
No compared value is a NaN."""
import numpy as np
import pytest

from tests import orient_model as OM
from tests import orient_stress_cases as SC
from tests import points_knn_model as KM

f32, f64 = np.float32, np.float64


def _u(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _flipped(c, out):
    """The indices whose normal came back with its sign bits flipped; asserts that every other came back as it was."""
    nrm = c["normals"]
    flip = (_u(out) == (_u(nrm) ^ np.uint32(0x80000000))).all(axis=1) & OM.valid(nrm)
    assert np.array_equal(_u(out[~flip]), _u(nrm[~flip]))
    return np.nonzero(flip)[0]


# ---- 1. the seed search past one trip ----
def test_the_long_lines_reach_into_the_second_trip_of_the_seed_search():
    assert SC.seed_grid() == SC.TRIP and SC.LINE == SC.TRIP + 40 and SC.TIE_LOW < SC.TRIP <= SC.TIE_HIGH < SC.LINE


def test_line_rows_are_the_brute_force_rows():
    P = np.zeros((50, 3), f32)
    P[:, 2] = np.arange(50)
    idx, _, found = KM.knn(P, P, 3)
    assert np.array_equal(idx, SC.line_rows(50)[0]) and (found == 3).all()
    assert np.array_equal(SC.window_rows(P, 3, 3, 16.0)[0], idx)
    # the long line itself, at a few queries against every point
    c = SC.line()
    q = np.array([0, 1, 110, SC.TRIP - 1, SC.TRIP, SC.LINE - 2, SC.LINE - 1])
    idx, _, found = KM.knn(c["P"], c["P"][q], 3)
    assert np.array_equal(idx, c["rows"][0][q]) and (found == 3).all()
    c = SC.tie_across_trips()
    q = np.array([0, SC.TIE_LOW - 1, SC.TIE_LOW, SC.TIE_LOW + 1, SC.TIE_HIGH - 1, SC.TIE_HIGH, SC.TIE_HIGH + 1, SC.LINE - 1])
    idx, _, found = KM.knn(c["P"], c["P"][q], 3)
    assert np.array_equal(idx, c["rows"][0][q]) and (found == 3).all()


def test_line_takes_two_seeds_the_first_in_the_second_trip():
    c = SC.line()
    ok = OM.valid(c["normals"])
    assert np.array_equal(np.nonzero(ok)[0], np.concatenate(SC.LINE_VALID))
    assert OM.next_seed(c["P"][:, 2], ok) == SC.LINE - 1 >= SC.TRIP
    out, st = SC.model(c)
    assert st["seeds"] == 2 and st["unreached"] == 0 and st["invalid"] == SC.LINE - 50 and sum(st["levels"]) == 48
    assert 0 < st["flipped"] < 50
    # the first seed is the last point: with one seed only the last 30 are oriented and 100 .. 119 are not
    one = dict(c, max_seeds=1)
    out1, st1 = SC.model(one)
    assert st1["seeds"] == 1 and st1["unreached"] == 20 and np.array_equal(_u(out1[100:120]), _u(c["normals"][100:120]))
    assert np.array_equal(_u(out1[-30:]), _u(out[-30:])) and out[-1, 2] > 0 and out[119, 2] > 0


def test_equal_z_across_trips_the_lower_index_is_the_seed():
    c = SC.tie_across_trips()
    P, ok = c["P"], OM.valid(c["normals"])
    assert P[SC.TIE_LOW, 2] == P[SC.TIE_HIGH, 2] == P[:, 2].max() and (P[:, 2] == P[:, 2].max()).sum() == 2
    assert OM.next_seed(P[:, 2], ok) == SC.TIE_LOW
    out, st = SC.model(c)
    assert st["seeds"] == 1 and st["unreached"] == 7 and st["flipped"] == 7
    assert np.array_equal(_flipped(c, out), np.arange(SC.TIE_LOW - 3, SC.TIE_LOW + 4))      # (the other seed would flip the other seven)


# ---- 2. the deciding launch at a batch edge ----
def test_ladders_put_the_deciding_launch_around_the_batch_edges():
    B = SC.batch()
    cases = SC.ladders_at_batch_edges()
    assert sorted(cases) == [(b, d) for b in (1, 2) for d in (-1, 0, 1, 2)]
    for (b, d), c in cases.items():
        stations = len(c["P"]) // 2
        _, st = SC.model(c)
        assert st["rounds"] == stations + 5 and st["rounds"] + 1 == 1 + b * B + d        # a station per round, the seed, four empty levels
        assert st["seeds"] == 1 and st["unreached"] == 0 and st["levels"] == [2 * stations - 1, 0, 0, 0]
    assert sorted(len(c["P"]) // 2 for c in cases.values()) == [B - 6, B - 5, B - 4, B - 3, 2 * B - 6, 2 * B - 5, 2 * B - 4, 2 * B - 3]


# ---- 3. weights on the level thresholds ----
def test_threshold_chain_accepts_a_link_at_every_level_and_zeros_keep_their_normal():
    c = SC.threshold_chain()
    dots = SC.threshold_dots()
    n = len(c["P"])
    idx, _, found = KM.knn(c["P"], c["P"], 2)
    assert np.array_equal(idx[1:], np.stack([np.arange(1, n), np.arange(0, n - 1)], axis=1)) and list(idx[0]) == [0, 1]
    link = OM.dot(c["normals"][1:], c["normals"][:-1])                 # link i - 1 -> i
    assert np.array_equal(link, np.repeat(dots.astype(f64), 2))
    for t in OM.LEVELS[:3]:                                               # each threshold itself and the float32 next below it
        assert (np.abs(link) == t).any() and (np.abs(link) == f64(np.nextafter(f32(t), f32(0)))).any()
    out, st = SC.model(c)
    w = np.abs(link)
    want = [int((w >= 0.9375).sum()), int(((w < 0.9375) & (w >= 0.75)).sum()), int(((w < 0.75) & (w >= 0.5)).sum()), int((w < 0.5).sum())]
    assert st["levels"] == want and min(want) >= 4 and st["seeds"] == 1 and st["unreached"] == 0
    assert st["rounds"] == 1 + (n - 1) + 4                              # one link per round; an empty round before each level and at the end
    # the sign of a point is the product of the signs of the links before it, a zero of either sign counting as +
    sign = np.concatenate([[1], np.cumprod(np.where(link < 0, -1, 1))])
    assert np.array_equal(_flipped(c, out), np.nonzero(sign < 0)[0]) and (sign < 0).any()
    zero = np.nonzero(link == 0)[0] + 1                                  # the points reached over a link of exactly 0
    assert len(zero) == 4 and np.signbit(c["normals"][zero[2], 0]) and (sign[zero] == sign[zero - 1]).all()


# ---- 4. two sources of equal weight and opposite sign ----
def test_equal_weights_the_first_source_in_row_order_wins():
    results = []
    for exchanged in (False, True):
        c = SC.equal_weights(exchanged)
        idx, _, _ = KM.knn(c["P"], c["P"], 3)
        assert list(idx[3]) == [3, 1, 2]                                  # the target's sources in index order: their d2 are equal
        d = OM.dot(c["normals"][3], c["normals"][1:3])
        assert d[0] == -d[1] and abs(d[0]) == 0.5
        out, st = SC.model(c)
        assert st["rounds"] == 1 + 2 + 4 and st["levels"] == [2, 0, 1, 0] and st["unreached"] == 0
        assert np.array_equal(_u(out[:3]), _u(c["normals"][:3]))
        results.append(out[3, 0])
    assert results == [1.0, -1.0]


# ---- 5. small edges ----
def test_small_edges():
    c = SC.no_valid_normal()
    out, st = SC.model(c)
    assert st == {"rounds": 0, "seeds": 0, "flipped": 0, "unreached": 0, "invalid": 50, "levels": [0, 0, 0, 0]}
    assert np.array_equal(_u(out), _u(c["normals"]))
    c = SC.no_valid_normal(17)
    out, st = SC.model(c)
    assert st == {"rounds": 5, "seeds": 1, "flipped": 1, "unreached": 0, "invalid": 49, "levels": [0, 0, 0, 0]}
    assert list(_flipped(c, out)) == [17]
    for normal, flip in zip(SC.SEED_NORMALS, [0, 1, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 1]):
        c = SC.flat_seed(normal)
        out, st = SC.model(c)
        assert st["seeds"] == 1 and st["flipped"] == 3 * flip and sum(st["levels"]) == 2, normal
    x, y = np.abs(SC.SEED_NORMALS[:, 0]), np.abs(SC.SEED_NORMALS[:, 1])
    assert (x > y).any() and (x < y).any() and (x == y).any() and (SC.SEED_NORMALS[:, 2] == 0).all()
    for max_seeds in (1, 3, 64):
        c = SC.zero_z_ties(max_seeds)
        assert np.signbit(c["P"][0, 2]) and not np.signbit(c["P"][1, 2])
        out, st = SC.model(c)
        assert st["seeds"] == min(max_seeds, 12) and list(_flipped(c, out)) == list(range(min(max_seeds, 12)))


# ---- 6. max_distance = 0 ----
def test_triples_take_a_seed_per_distinct_point():
    c = SC.triples(500)
    _, _, found = KM.knn(c["P"], c["P"], 8, c["max_distance"])
    assert (found == 3).all()
    _, st = SC.model(c)
    assert st["seeds"] == 100 and st["unreached"] == 0 and sum(st["levels"]) == 200 and st["rounds"] >= 600
    _, st = SC.model(SC.triples(64))
    assert st["seeds"] == 64 and st["unreached"] == 108


# ---- 7. scaled clouds ----
@pytest.mark.parametrize("e", SC.SCALES)
def test_scaled_spheres_still_orient(e):
    c = SC.scaled_sphere(e)
    out, st = SC.model(c)
    assert st["seeds"] >= 1 and st["invalid"] == 0 and 0 < st["flipped"] < len(out)
    if e == -70:                                                          # the d2 are subnormal: the rows are not the unscaled cloud's
        _, d, _ = KM.knn(c["P"], c["P"][:50], 8)
        assert 0 < (d.astype(f64) ** 2).max() < 2.0 ** -126
