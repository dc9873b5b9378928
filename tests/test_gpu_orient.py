"""KdTree.OrientNormals on the MI355X against the numpy model (tests/orient_model.py).  Every comparison is bit for bit: normals as
uint32, stats equal to the model's."""
import ctypes as C

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from tests import orient_cases as OC
from tests import orient_model as OM
from tests import pointcloud_model as PC
from tests import scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = np.inf
KS = [2, 8, 9, 16, 33]           # the register tier at its edge, and the LDS tiers 16 and 64
BATCH = 32                       # rounds queued between two reads of the control block (csrc/lib_orient.hip kBatch)


def _u(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _exact(tree, P, nrm, k=8, max_distance=INF, max_seeds=64):
    """OrientNormals == the model, normals and stats -> (normals, stats)."""
    stats = {}
    got = tree.OrientNormals(nrm, k, max_distance, max_seeds, stats)
    want, st = OM.orient(P, nrm, k, max_distance, max_seeds)
    assert got.shape == want.shape and got.dtype == f32
    bad = np.nonzero((_u(got) != _u(want)).any(axis=1))[0]
    assert len(bad) == 0, (k, len(bad), bad[:3], got[bad[:3]], want[bad[:3]], stats, st)
    assert stats == st, (stats, st)
    return got, stats


_cache = {}


def _data(name):
    """name -> (tree, static points, unoriented normals from EstimateNormals without a viewpoint), made once."""
    if name in _cache:
        return _cache[name]
    rs = np.random.default_rng(61)
    if name == "uniform":                     # more than one block; the normals are garbage, the decisions must still match
        P = rs.random((5000, 3), dtype=f32)
    elif name in OC.CASES:
        P = np.array(OC.cloud(name)[0])
    elif name == "mesh":                      # the vertices of a catalogue mesh at 40^3
        _, sdf = S.CATALOGUE["cylinder"]()
        m = sdf.ToMesh([-2.5] * 3, [2.5] * 3, 40, 40, 40, clipToBounds=False)
        P = np.ascontiguousarray(np.asarray(m.Vertices, f32).reshape(-1, 3))
    elif name == "lattice":                   # mass ties
        g = np.arange(9, dtype=f32)
        P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)
        P = P[rs.permutation(len(P))]
    elif name == "two_batches":
        P = (rs.standard_normal((3000, 3)) * 0.3).astype(f32)
    if name == "two_batches":
        tree = K.KdTree(P[:1700])
        tree.AddPoints(P[1700:])
    else:
        tree = K.KdTree(P)
    assert tree.TotalPoints == len(P)
    nrm, _ = tree.EstimateNormals(OC.CASES[name][1] if name in OC.CASES else 8)
    _cache[name] = (tree, P, nrm)
    return _cache[name]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["uniform", "sphere", "torus", "cube", "mesh", "lattice", "two_batches"])
def test_orientation_equals_the_model(gpu, name, k):
    tree, P, nrm = _data(name)
    got, stats = _exact(tree, P, nrm, k)
    assert np.array_equal(_u(got) & np.uint32(0x7fffffff), _u(nrm) & np.uint32(0x7fffffff))   # the input up to sign
    assert stats["invalid"] == 0 and stats["seeds"] >= 1 and stats["rounds"] >= stats["seeds"] + 4


def test_more_rounds_than_one_queued_batch(gpu):
    tree, P, nrm = _data("strip")
    got, stats = _exact(tree, P, nrm, OC.CASES["strip"][2])
    assert stats["rounds"] > 2 * BATCH and stats["seeds"] == 1 and stats["unreached"] == 0
    assert OC.fraction_right(got, OC.cloud("strip")[1], closed=False) == 1.0


@pytest.mark.parametrize("count", [2, 3])
def test_far_clusters_take_a_seed_each(gpu, count):
    P, out = OC.clusters(count)
    tree = K.KdTree(P)
    nrm, _ = tree.EstimateNormals(8)
    got, stats = _exact(tree, P, nrm)
    assert stats["seeds"] == count and stats["unreached"] == 0 and (np.einsum("ij,ij->i", got, out) > 0).all()
    if count == 2:                            # one seed only: the second cluster is untouched
        got, stats = _exact(tree, P, nrm, max_seeds=1)
        assert stats["seeds"] == 1 and stats["unreached"] == 400 and np.array_equal(_u(got[400:]), _u(nrm[400:]))
        assert (np.einsum("ij,ij->i", got[:400], out[:400]) > 0).all()


def test_a_finite_max_distance_isolates_points(gpu):
    rs = np.random.default_rng(62)
    P = np.concatenate([OC.fibonacci(600), (rs.random((7, 3)) * 4 + 3).astype(f32)]).astype(f32)
    nrm = np.concatenate([OC.fibonacci(600) * rs.choice([-1, 1], (600, 1)), rs.standard_normal((7, 3))]).astype(f32)
    tree = K.KdTree(P)
    got, stats = _exact(tree, P, nrm, 8, f32(0.5))
    assert stats["seeds"] == 8 and stats["unreached"] == 0 and (np.einsum("ij,ij->i", got[:600], P[:600]) > 0).all()
    got, stats = _exact(tree, P, nrm, 8, f32(0.5), max_seeds=3)
    assert stats["seeds"] == 3 and stats["unreached"] > 0


@pytest.mark.parametrize("name", ["cube", "plate"])
def test_levels_equal_the_model(gpu, name):
    tree, P, nrm = _data(name)
    got, stats = _exact(tree, P, nrm, OC.CASES[name][2])
    assert sum(1 for c in stats["levels"] if c) >= 2 and sum(stats["levels"]) + stats["seeds"] == len(P)
    assert OC.fraction_right(got, OC.cloud(name)[1]) >= 0.99
    assert np.array_equal(_u(nrm), _u(OC.cloud(name)[2]))       # (EstimateNormals is the model's: the recorded figures are these)


def test_invalid_normals_are_returned_and_are_no_bridges(gpu):
    rs = np.random.default_rng(63)
    # two spheres joined by a line of points: with normals the line is a bridge, without them it is not
    A, B = OC.fibonacci(500), OC.fibonacci(500, 1.0, (5.0, 0.0, -0.5))
    line = np.stack([np.linspace(1.05, 3.95, 60), np.zeros(60), np.full(60, -0.02)], axis=1).astype(f32)
    P = np.concatenate([A, line, B]).astype(f32)
    nrm = np.concatenate([A * rs.choice([-1, 1], (500, 1)), np.tile([[0, 0, 1]], (60, 1)), OC.fibonacci(500) * rs.choice([-1, 1], (500, 1))]).astype(f32)
    tree = K.KdTree(P)
    _, stats = _exact(tree, P, nrm)
    assert stats["seeds"] == 1
    bad = np.array([[0, 0, 0], [-0.0, 0, -0.0], [np.nan, 0, 1], [0, np.inf, 0], [1, 0, -np.inf]], f32)
    nrm[500:560] = bad[rs.integers(0, len(bad), 60)]
    scattered = rs.choice(500, 40, replace=False)
    nrm[scattered] = bad[rs.integers(0, len(bad), 40)]
    got, stats = _exact(tree, P, nrm)
    assert stats["seeds"] == 2 and stats["invalid"] == 100 and stats["unreached"] == 0
    assert np.array_equal(_u(got[500:560]), _u(nrm[500:560])) and np.array_equal(_u(got[scattered]), _u(nrm[scattered]))
    ok = OM.valid(nrm)
    centre = np.where(np.arange(len(P))[:, None] < 560, 0.0, np.array([5.0, 0.0, -0.5]))
    assert (np.einsum("ij,ij->i", got[ok], (P - centre)[ok]) > 0).all()


def test_duplicates_tiny_sets_and_refusals(gpu):
    rs = np.random.default_rng(64)
    for n, k in ((1, 2), (2, 2), (2, 8), (5, 8), (5, 33)):
        P = rs.random((n, 3), dtype=f32)
        nrm = rs.standard_normal((n, 3)).astype(f32)
        _, stats = _exact(K.KdTree(P), P, nrm, k)
        assert stats["unreached"] == 0
    P = np.tile(np.array([[0.25, 0.5, 0.75]], f32), (40, 1))            # every point a duplicate: each row is the first k indices
    for k in (2, 8, 16):
        _exact(K.KdTree(P), P, rs.standard_normal((40, 3)).astype(f32), k)
    tree, P, nrm = _data("sphere")
    for bad in dict(k=1), dict(k=65), dict(k=0), dict(maxDistance=np.nan), dict(maxDistance=-1.0), dict(maxSeeds=0), dict(maxSeeds=-3):
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.OrientNormals(nrm, **bad)
        assert e.value.status == N.ERR_INVALID
    st = (C.c_int64 * 9)()
    assert N.lib().sdfk_points_orient_normals(tree.handle, 8, float(INF), 64, None, st) == N.ERR_INVALID
    with pytest.raises(ValueError):
        tree.OrientNormals(nrm[:5])
    # the empty set: a set always holds a point (sdfk_points_create refuses none), so there is nothing to orient in one
    with pytest.raises(N.SdfKitNativeError) as e:
        K.KdTree(np.zeros((0, 3), f32))
    assert e.value.status == N.ERR_INVALID


def test_properties(gpu):
    tree, P, nrm = _data("sphere")
    got = tree.OrientNormals(nrm)
    assert np.array_equal(_u(got) & np.uint32(0x7fffffff), _u(nrm) & np.uint32(0x7fffffff))
    assert (np.einsum("ij,ij->i", got, P) > 0).all() and not (np.einsum("ij,ij->i", nrm, P) > 0).all()
    assert np.array_equal(_u(tree.OrientNormals(got)), _u(got))             # applying it twice changes nothing
    assert np.array_equal(_u(tree.OrientNormals(-nrm)), _u(got))            # globally negated input: the same output
    rs = np.random.default_rng(65)
    analytic = (P * rs.choice([-1, 1], (len(P), 1))).astype(f32)           # analytic normals, signs at random
    back, stats = _exact(tree, P, analytic)
    assert (np.einsum("ij,ij->i", back, P) > 0).all() and stats["flipped"] == int((analytic[:, 0] != P[:, 0]).sum())


def test_device_form_equals_the_host_form(gpu):
    import torch
    tree, P, nrm = _data("torus")
    stats = {}
    host = tree.OrientNormals(nrm, 9, stats=stats)
    N.bind_torch_stream()
    nd = torch.from_numpy(nrm.copy()).to(torch.device("cuda:0"))
    st = (C.c_int64 * 9)()
    N.check(N.lib().sdfk_points_orient_normals_device(tree.handle, 9, float(INF), 64, C.c_void_p(nd.data_ptr()), st))
    N.check(N.lib().sdfk_synchronize())
    torch.cuda.synchronize()
    assert np.array_equal(_u(nd.cpu().numpy()), _u(host))
    assert [int(v) for v in st] == [stats["rounds"], stats["seeds"], stats["flipped"], stats["unreached"], stats["invalid"]] + stats["levels"]
    N.check(N.lib().sdfk_set_stream(None))


def test_end_to_end_sphere_without_a_viewpoint(gpu):
    """What the feature is for: EstimateNormals without a viewpoint -> OrientNormals -> ToVoxels gives the sphere's volume; the
    unoriented normals do not."""
    tree, P, nrm = _data("sphere")
    box, n = ([-1.5] * 3, [1.5] * 3), 32
    band = f32(3 * 3.0 / n)
    oriented = tree.OrientNormals(nrm, 8)
    model_oriented, _ = OM.orient(P, PC.normals(P, 8)[0], 8)
    assert np.array_equal(_u(oriented), _u(model_oriented))
    vox = tree.ToVoxels(oriented, *box, n, n, n, k=8, maxDistance=band).Values
    want, _ = PC.to_volume(P, model_oriented, *box, (n, n, n), 8, band)
    assert np.array_equal(_u(vox), _u(want))
    corners = [(i, j, k) for i in (0, n - 1) for j in (0, n - 1) for k in (0, n - 1)]
    assert vox[n // 2, n // 2, n // 2] < 0 and all(vox[c] > 0 for c in corners)
    raw = tree.ToVoxels(nrm, *box, n, n, n, k=8, maxDistance=band).Values
    assert not (raw[n // 2, n // 2, n // 2] < 0 and all(raw[c] > 0 for c in corners))     # the gap being closed
