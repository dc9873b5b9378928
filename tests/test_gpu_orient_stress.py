"""KdTree.OrientNormals on the MI355X on the clouds of tests/orient_stress_cases.py against the numpy model (tests/orient_model.py):
a seed search that takes a second trip, the growth ending on either side of a queued batch, weights on the level thresholds, two
sources of equal weight, clouds without a valid normal, max_distance = 0 and scaled clouds, in the host and the device form.  Every
comparison is bit for bit: normals as uint32, all nine stats equal to the model's.  What the clouds are there for is proved on the
CPU in tests/test_orient_stress_cases.py; no compared value is a NaN unless the input holds it."""
import ctypes as C

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from tests import orient_stress_cases as SC
from tests.test_gpu_orient import BATCH, _u

pytestmark = pytest.mark.gpu
f32 = np.float32


def _stats_list(st):
    return [st["rounds"], st["seeds"], st["flipped"], st["unreached"], st["invalid"]] + st["levels"]


def _exact(c, tree=None):
    """OrientNormals on a case == the model, normals and all nine stats -> (normals, stats, tree)."""
    tree = tree or K.KdTree(c["P"])
    stats = {}
    got = tree.OrientNormals(c["normals"], c["k"], c["max_distance"], c["max_seeds"], stats)
    want, st = SC.model(c)
    assert got.shape == want.shape and got.dtype == f32
    bad = np.nonzero((_u(got) != _u(want)).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:3], got[bad[:3]], want[bad[:3]], stats, st)
    assert _stats_list(stats) == _stats_list(st), (stats, st)
    return got, stats, tree


def _rows_equal_the_search(tree, c):
    """SearchKNearest on about 1000 sampled points returns the closed-form rows: a difference there is not one of the orientation."""
    q = SC.sample_indices(len(c["P"]))
    idx, _, found = tree.SearchKNearest(c["P"][q], c["k"])
    assert np.array_equal(idx, c["rows"][0][q]) and np.array_equal(found, c["rows"][1][q])


@pytest.fixture(scope="module")
def line(gpu):
    c = SC.line()
    return c, K.KdTree(c["P"])


# ---- 1. the seed search past one trip ----
def test_seed_in_the_second_trip_of_the_search(line):
    c, tree = line
    _rows_equal_the_search(tree, c)
    got, stats, _ = _exact(c, tree)
    assert stats["seeds"] == 2 and stats["unreached"] == 0 and got[-1, 2] > 0
    _, stats, _ = _exact(dict(c, max_seeds=1), tree)                    # the first seed is the last point
    assert stats["seeds"] == 1 and stats["unreached"] == 20


def test_equal_z_in_both_trips_the_lower_index_is_the_seed(gpu):
    c = SC.tie_across_trips()
    tree = K.KdTree(c["P"])
    _rows_equal_the_search(tree, c)
    got, stats, _ = _exact(c, tree)
    assert stats["seeds"] == 1 and stats["flipped"] == 7 and got[SC.TIE_LOW, 2] == 1 and got[SC.TIE_HIGH, 2] == -1


# ---- 2. the deciding launch at a batch edge ----
@pytest.mark.parametrize("b,d", [(b, d) for b in (1, 2) for d in (-1, 0, 1, 2)])
def test_growth_ending_around_a_batch_edge(gpu, b, d):
    assert SC.batch() == BATCH
    c = SC.ladders_at_batch_edges()[(b, d)]
    _, stats, _ = _exact(c)
    assert stats["rounds"] + 1 == 1 + b * BATCH + d and stats["seeds"] == 1 and stats["unreached"] == 0


# ---- 3. and 4. thresholds and ties through the kernel ----
def test_weights_on_the_level_thresholds(gpu):
    _, stats, _ = _exact(SC.threshold_chain())
    assert min(stats["levels"]) >= 4 and stats["seeds"] == 1 and stats["unreached"] == 0


@pytest.mark.parametrize("exchanged", [False, True])
def test_equal_weights_the_first_source_in_row_order_wins(gpu, exchanged):
    got, stats, _ = _exact(SC.equal_weights(exchanged))
    assert got[3, 0] == (-1 if exchanged else 1) and stats["levels"] == [2, 0, 1, 0]


# ---- 5. small edges ----
def test_no_valid_normal_and_exactly_one(gpu):
    c = SC.no_valid_normal()
    got, stats, tree = _exact(c)
    assert _stats_list(stats) == [0, 0, 0, 0, 50, 0, 0, 0, 0] and np.array_equal(_u(got), _u(c["normals"]))
    _, stats, _ = _exact(SC.no_valid_normal(17), tree)
    assert _stats_list(stats) == [5, 1, 1, 0, 49, 0, 0, 0, 0]


def test_seed_normals_without_a_z_component(gpu):
    tree = None
    for normal in SC.SEED_NORMALS:
        _, stats, tree = _exact(SC.flat_seed(normal), tree)
        assert stats["seeds"] == 1 and stats["flipped"] in (0, 3)


def test_seeds_of_equal_z_of_either_zero_come_in_index_order(gpu):
    tree = None
    for max_seeds in (1, 3, 64):
        got, stats, tree = _exact(SC.zero_z_ties(max_seeds), tree)
        assert stats["seeds"] == min(max_seeds, 12) and (got[:stats["seeds"], 2] == 1).all() and (got[stats["seeds"]:, 2] == -1).all()


# ---- 6. max_distance = 0 ----
def test_max_distance_zero_and_more_seeds_than_the_default_cap(gpu):
    c = SC.triples(500)
    _, stats, tree = _exact(c)
    assert stats["seeds"] == 100 and stats["unreached"] == 0 and stats["rounds"] >= 600
    stats = {}
    tree.OrientNormals(c["normals"], c["k"], c["max_distance"], stats=stats)       # the member's default: 64 seeds
    want = SC.model(SC.triples(64))[1]
    assert _stats_list(stats) == _stats_list(want) and stats["seeds"] == 64 and stats["unreached"] == 108
    _exact(SC.triples(64), tree)


# ---- 7. scaled clouds ----
@pytest.mark.parametrize("e", SC.SCALES)
def test_scaled_spheres(gpu, e):
    _, stats, _ = _exact(SC.scaled_sphere(e))
    assert stats["seeds"] >= 1 and stats["invalid"] == 0


# ---- 8. the device form ----
def test_device_form_on_the_long_line(line):
    import torch
    c, tree = line
    want, st = SC.model(c)
    N.bind_torch_stream()
    try:
        nd = torch.from_numpy(c["normals"].copy()).to(torch.device("cuda:0"))
        got = (C.c_int64 * 9)()
        N.check(N.lib().sdfk_points_orient_normals_device(tree.handle, c["k"], float(c["max_distance"]), c["max_seeds"], C.c_void_p(nd.data_ptr()), got))
        N.check(N.lib().sdfk_synchronize())
        torch.cuda.synchronize()
        assert np.array_equal(_u(nd.cpu().numpy()), _u(want))
        assert [int(v) for v in got] == _stats_list(st)
    finally:
        N.check(N.lib().sdfk_set_stream(None))
