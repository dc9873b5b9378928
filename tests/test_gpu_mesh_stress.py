"""The mesh units on the MI355X on the stress cases (tests/mesh_stress_cases.py; what each case is there for is proved from the
models alone in tests/test_mesh_stress_cases.py): topology (csrc/lib_trimesh_topology.hip), adjacency, smoothing and vertex
normals (csrc/lib_trimesh_smooth.hip), welding (csrc/lib_trimesh_weld.hip) and Mesh.SamplePoints (csrc/lib_trimesh.hip) against
their numpy models.  The tidy meshes of the units' own GPU tests keep every run of sorted records short; here are random index
soups, 300 of them laid over each other, one edge of 5000 triangles, hubs of 5001 neighbours and 5000 corners, hubs whose sums
cancel so that only the stated order of the adds gives the model's bits, 70 000 components, one weld group of 6050 vertices and
the lattice's cell faces at zero and below.  Everything is compared with np.array_equal on integers or float bits -- nothing
here has a tolerance -- by the comparisons of the units' own tests, imported from them."""
import functools

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import MeshSdf
from tests import mesh_sample_model as SM
from tests import mesh_smooth_model as AM
from tests import mesh_stress_cases as SC
from tests import mesh_topology_model as TM
from tests.mesh_weld_cases import FLAGS, index_colors
from tests.test_gpu_mesh_sample import _same as _same_samples
from tests.test_gpu_mesh_smooth import TAUBIN, _bits, _check_adjacency
from tests.test_gpu_mesh_topology import _check as _check_topology
from tests.test_gpu_mesh_topology import _check_selection
from tests.test_gpu_mesh_weld import _check as _check_weld

pytestmark = pytest.mark.gpu
f32 = np.float32


def _check_smooth_and_normals(t, V, T, adj, what, runs):
    """runs: (iterations, lambda, mu, pin) each; then the normals of the handle's own positions."""
    for k, lam, mu, pin in runs:
        got = t.Smooth(k, lam, mu, pin)
        assert got.dtype == f32 and np.array_equal(_bits(got), _bits(AM.smooth(V, T, k, lam, mu, pin, adj=adj))), (what, k, lam, mu, pin)
    cor = AM.corners(len(V), T)
    want = AM.vertex_normals(V, T, cor=cor)
    assert np.array_equal(_bits(t.VertexNormals()), _bits(want)), what
    return cor, want


# ---- the soups: one test per unit, over the 64 seeds ----------------------------------------------------------------------------
def test_soups_topology(gpu):
    for s in SC.SOUP_SEEDS:
        V, T = SC.soup(s)
        _check_topology(V, T, what=("soup", s), keeps=([True], [False], [True, False]))


def test_soups_adjacency_smoothing_and_normals(gpu):
    for s in SC.SOUP_SEEDS:
        V, T = SC.soup(s)
        t = MeshSdf((V, T))
        adj = _check_adjacency(t, V, T, ("soup", s))
        cor, _ = _check_smooth_and_normals(t, V, T, adj, ("soup", s), [(k,) + TAUBIN + (pin,) for k in (0, 1, 2) for pin in (True, False)])
        assert np.array_equal(_bits(t.VertexNormals(flip=True)), _bits(AM.vertex_normals(V, T, flip=True, cor=cor))), s


def test_soups_weld(gpu):
    for s in SC.SOUP_SEEDS:
        V, T = SC.soup(s)
        for tol in (0.0, 0.25, 0.6):
            _check_weld(V, T, None, tol, ("soup", s, tol), flag_set=FLAGS, raw_flags=())


def test_soups_sampling(gpu):
    refused = 0
    for s in SC.SOUP_SEEDS:
        V, T = SC.soup(s)
        t = MeshSdf((V, T))
        if SM.weights(V, T)[0] is None:
            refused += 1
            with pytest.raises(N.SdfKitNativeError, match="no triangle has an area"):
                t.SamplePoints(257, s)
            continue
        for strat in (True, False):
            _same_samples(t.SamplePoints(257, s, stratified=strat), SM.sample(V, T, 257, s, strat), ("soup", s, strat))
    assert refused >= 1


# ---- the archipelago ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _archipelago():
    V, T = SC.archipelago()
    return V, T, index_colors(len(V)), TM.topology(V, T)


def test_archipelago_topology_and_cleaning(gpu):
    V, T, cols, want = _archipelago()
    rng = np.random.default_rng(41)
    keep = rng.integers(0, 2, want.count) == 1
    t, _, c = _check_topology(V, T, colors=cols, what="archipelago", keeps=(keep, [True], [False]))
    assert c.Count == want.count >= 300 and np.all(c.Rows.sum(axis=0)[2:7] > 0)
    # Mesh.RemoveSmallComponents at the median triangle count: some components go, some stay
    least = int(np.median(want.rows[:, 0])) + 1
    small = TM.keep_small_removed(want.rows, least)
    assert 0 < np.count_nonzero(small) < want.count
    s = TM.select(V, T, small, colors=cols, topo=want)
    m = K.Mesh(V, cols, np.zeros_like(V), T.reshape(-1)).RemoveSmallComponents(minTriangles=least)
    assert np.array_equal(np.asarray(m.Triangles), s.triangles) and np.array_equal(_bits(m.Vertices), _bits(s.vertices))
    assert np.array_equal(_bits(m.Colors), _bits(s.colors))
    _check_selection(t.Select(small), s, "small removed")


@pytest.mark.parametrize("tol", [0.0, 0.25])
def test_archipelago_weld(gpu, tol):
    V, T, cols, _ = _archipelago()
    _, out = _check_weld(V, T, cols, tol, ("archipelago", tol), flag_set=(0, 3), raw_flags=(0, 3))   # (raw: the host and the _device form)
    assert out[0].merged > 1000 and out[0].degenerate > int(TM.degenerate(T).sum()) and out[0].unreferenced > 0


def test_archipelago_sampling_never_takes_a_triangle_without_weight(gpu):
    V, T, cols, _ = _archipelago()
    w, _ = SM.weights(V, T)
    assert np.count_nonzero(w == 0) > 0.15 * len(T)
    t = MeshSdf((V, T, cols))
    for strat in (True, False):
        got = t.SamplePoints(20011, 9, stratified=strat)
        _same_samples(got, SM.sample(V, T, 20011, 9, strat, colors=cols), ("archipelago", strat))
        assert np.all(w[got.Triangles] > 0)
    assert t.sample_stats() == {"sampled_triangles": int(np.count_nonzero(w)), "total_weight": int(w.sum())}


# ---- the books: runs of 5000 records --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.BOOKS))
def test_books(gpu, name):
    n, _ = SC.BOOKS[name]
    V, T = SC.book(*SC.BOOKS[name])
    t, want, c = _check_topology(V, T, what=name, keeps=([True], [False]))
    assert want.census.tolist() == SC.BOOK_CENSUS[name] and c.Count == 1 and c.Rows[0][:7].tolist() == [n] + SC.BOOK_CENSUS[name][1:7]
    adj = _check_adjacency(t, V, T, name)
    got = t.Adjacency()
    assert got.Degree[:2].tolist() == [n + 1, n + 1] and np.all(got.Degree[2:] == 2) and np.all(got.Boundary == 1)
    assert np.array_equal(got.Of(0), np.arange(1, n + 2)) and np.array_equal(got.Of(1), np.concatenate([[0], np.arange(2, n + 2)]))
    _check_smooth_and_normals(t, V, T, adj, name, [(1,) + TAUBIN + (False,), (2,) + TAUBIN + (False,)])


def test_cancelling_book_sums_in_the_stated_order(gpu):
    """The test of the stated order: neighbours ascending in k_tv_step, corners ascending in k_tv_normals.  In any other order the
    hubs' float32 results differ (tests/test_mesh_stress_cases.py shows it for the descending one).  The closest-point grid of
    the handle, which the spread of the radii sizes, is printed."""
    V, T = SC.cancelling_book()
    t = MeshSdf((V, T))
    st = t.stats()
    print("cancelling_book: closest-point grid", st["grid"], "triangle-cell pairs", st["entries"])
    adj = _check_adjacency(t, V, T, "cancelling_book")
    _, normals = _check_smooth_and_normals(t, V, T, adj, "cancelling_book", [(1, 0.5, 0.0, False)])
    got = t.Smooth(1, 0.5, 0.0, False)
    assert np.all(got[:2, :2] != 0) and np.all(np.any(normals[:2] != 0, axis=1))   # the residues of the hubs' sums: neither cancelled to 0


# ---- the large counts -----------------------------------------------------------------------------------------------------------
def test_loose_triangles_more_components_than_65536(gpu):
    V, T = SC.loose_triangles()
    keep = np.random.default_rng(42).integers(0, 2, len(T)) == 1
    _, want, c = _check_topology(V, T, what="loose_triangles", keeps=(keep,))      # (every one of the 70 000 rows, the census, Select)
    assert c.Count == want.count == 70000 > 65536


@pytest.mark.parametrize("tol", [0.0, 0.5])
def test_one_big_group(gpu, tol):
    V, T = SC.one_big_group()
    _, out = _check_weld(V, T, index_colors(len(V)), tol, ("one_big_group", tol), flag_set=FLAGS, raw_flags=FLAGS)
    size = np.bincount(out[0].rep)
    assert size.max() > 2 * 2048 and out[0].rep[np.flatnonzero(out[0].rep == size.argmax())].min() == size.argmax()


def test_negative_faces(gpu):
    tol = SC.NEGATIVE_FACES_TOLERANCE
    V, T = SC.negative_faces(tol)
    t, _ = _check_weld(V, T, None, tol, "negative_faces", flag_set=FLAGS, raw_flags=(0, 3))
    vm = t.Weld(tol, True, True).VertexMap
    assert np.all(vm >= 0)
    for a in range(3):
        for k in SC.FACE_KS:
            on, below, above = (SC.face_vertex(a, k, s) for s in range(3))
            assert vm[on] == vm[above] and vm[below] != vm[on], (a, k)
        assert vm[SC.minus_zero_vertex(a)] == vm[SC.face_vertex(a, 0, 0)], a

