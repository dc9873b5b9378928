"""The mesh stress cases (tests/mesh_stress_cases.py) against the numpy models alone, on the CPU: every case has the property it is
there for, and each of twelve named wrong variants of a model -- a few lines over the model's own intermediate arrays, below --
gives a result that differs from the model's on at least one case.  What the device does with the cases is
tests/test_gpu_mesh_stress.py; a case that lost its property would make that test pass for nothing."""
import functools
import math

import numpy as np
import pytest

from tests import mesh_smooth_model as AM
from tests import mesh_stress_cases as SC
from tests import mesh_topology_model as TM
from tests import mesh_weld_model as WM

f32, f64, i32, i64, u32 = np.float32, np.float64, np.int32, np.int64, np.uint32


def _u(a):
    return np.ascontiguousarray(a, f32).view(u32)


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (V, T): every case but the 70 000 loose triangles (which no variant needs)."""
    out = {("soup", s): SC.soup(s) for s in SC.SOUP_SEEDS}
    out["archipelago"] = SC.archipelago()
    for name, args in SC.BOOKS.items():
        out[("book", name)] = SC.book(*args)
    out["cancelling_book"] = SC.cancelling_book()
    out["one_big_group"] = SC.one_big_group()
    out["negative_faces"] = SC.negative_faces()
    return out


@functools.lru_cache(maxsize=None)
def _topology(name):
    return TM.topology(*_cases()[name])


def _differs_on(variant, names=None):
    """The cases on which variant(V, T) -> (the variant's result, the model's) gives two different results."""
    return [n for n in (names or _cases()) if not _equal(*variant(*_cases()[n]))]


def _equal(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


# ---- every case is a mesh the library accepts -----------------------------------------------------------------------------------
def test_every_case_is_accepted_at_creation():
    meshes = dict(_cases())
    meshes["loose_triangles"] = SC.loose_triangles()
    for name, (V, T) in meshes.items():
        assert V.dtype == f32 and T.dtype == i32 and V.shape[1:] == (3,) and T.shape[1:] == (3,), name
        assert len(T) >= 1 and len(V) >= 1 and np.all(np.isfinite(V)), name
        assert T.min() >= 0 and T.max() < len(V), name


def test_the_cases_are_the_same_on_every_call():
    for make in (lambda: SC.soup.__wrapped__(5), SC.archipelago.__wrapped__, lambda: SC.cancelling_book.__wrapped__(),
                 lambda: SC.one_big_group.__wrapped__(), lambda: SC.loose_triangles.__wrapped__(2000)):
        (V, T), (W, S) = make(), make()
        assert np.array_equal(_u(V), _u(W)) and np.array_equal(T, S)


# ---- the soups ------------------------------------------------------------------------------------------------------------------
def test_soups_have_what_they_are_there_for():
    total = np.zeros(8, i64)
    most_edges, most_components, late_degenerate, listed_again, minus_zero = 0, 0, 0, 0, 0
    assert len(SC.SOUP_SEEDS) == 64
    for s in SC.SOUP_SEEDS:
        V, T = SC.soup(s)
        assert 3 <= len(V) < 40 and len(T) >= 1
        assert np.all(np.abs(V) <= 1) and np.array_equal(V * 4, np.round(V * 4))
        t = _topology(("soup", s))
        total += t.census
        vertex, tri, count = TM.labels_union_find(len(V), T)
        assert np.array_equal(t.vertex, vertex) and np.array_equal(t.triangle, tri) and t.count == count, s
        _, m, _ = TM.edges(T)
        most_edges = max(most_edges, int(m.max()) if len(m) else 0)
        most_components = max(most_components, t.count)
        rep = WM.weld(V, T).rep
        late_degenerate += int(np.count_nonzero(WM.degenerate(rep[T]) & ~WM.degenerate(T)))
        listed_again += len(T) - len(np.unique(np.sort(T, axis=1), axis=0))
        minus_zero += int(np.count_nonzero(_u(V) == 0x80000000))
    assert np.all(total > 0), total                     # every census column, the degenerate and the inconsistent ones included
    assert most_edges >= 8 and most_components >= 3, (most_edges, most_components)
    assert late_degenerate > 0 and listed_again > 0 and minus_zero > 0


def test_archipelago():
    V, T = SC.archipelago()
    t = _topology("archipelago")
    assert t.count >= 300 and np.all(t.census > 0), t.census
    w = TM.area_weights(V, T)
    assert np.count_nonzero(w == 0) >= 0.15 * len(T) and np.count_nonzero(w) >= 1000
    # an index-degenerate triangle on a vertex that nothing else names, and a triangle degenerate only after the weld
    named = np.bincount(T[~TM.degenerate(T)].reshape(-1), minlength=len(V))
    assert np.any(named[T[TM.degenerate(T)]] == 0)
    weld = WM.weld(V, T)
    assert np.any(WM.degenerate(weld.rep[T]) & ~WM.degenerate(T))
    group = np.bincount(weld.rep, minlength=len(V))
    assert weld.merged > 1000 and group.max() >= 8
    # the components share positions: a position held by vertices of different components
    both = (t.vertex >= 0) & (t.vertex[weld.rep] >= 0)
    assert np.count_nonzero(t.vertex[both] != t.vertex[weld.rep][both]) > 1000
    assert int(AM.adjacency(len(V), T).degree.max()) >= 16


# ---- the books ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.BOOKS))
def test_books(name):
    n, _ = SC.BOOKS[name]
    V, T = SC.book(*SC.BOOKS[name])
    t = _topology(("book", name))
    assert t.census.tolist() == SC.BOOK_CENSUS[name] and t.rows[0][:7].tolist() == [n] + SC.BOOK_CENSUS[name][1:7]
    keys, m, f = TM.edges(T)
    assert keys[0] == 1 and m[0] == n and np.all(m[1:] == 1)           # the spine, (0, 1), sorts first
    adj, cor = AM.adjacency(len(V), T), AM.corners(len(V), T)
    assert adj.degree.tolist() == [n + 1, n + 1] + [2] * n and np.all(adj.boundary == 1)
    assert np.diff(cor.start.astype(i64)).tolist() == [n, n] + [1] * n
    if n > 2:
        assert 3 * n > n > 2 * 2048 and int(f[0]) not in (0, n, n - int(f[0]))   # a run of more than two sort tiles, wound both ways
        assert (n % 2 == 1) == (name == "odd_4999")


def test_cancelling_book_is_decided_by_the_order_of_the_adds():
    """(g) and (h): either hub's neighbours, or corners, summed in descending order give other float32 bits; the hubs' normals are
    not zero.  Everything else in the mesh is a vertex of two neighbours and one corner, where no order exists."""
    V, T = SC.cancelling_book()
    h = SC.CANCELLING_HALF
    nv = len(V)
    assert nv == 2 * h + 2 and len(T) == 2 * h
    ring = V[2:].astype(f64)
    assert math.fsum(ring[:, 0]) == 0 and math.fsum(ring[:, 1]) == 0   # the exact sums (numpy's own rounded sum is not 0: the point)
    partner = {tuple(p) for p in ring.tolist()}
    assert all((-x, -y, z) in partner for x, y, z in ring.tolist())
    assert np.any(np.diff(np.lexsort(ring.T[::-1])) < 0)               # the indices are permuted
    adj, cor = AM.adjacency(nv, T), AM.corners(nv, T)
    assert adj.degree[:2].tolist() == [2 * h + 1] * 2 and np.diff(cor.start.astype(i64))[:2].tolist() == [2 * h] * 2
    assert 2 * h > 2048
    step, normals = AM.step(V, adj, 0.5), AM.vertex_normals(V, T, cor=cor)
    for hub in (0, 1):
        assert np.any(normals[hub] != 0) and normals[hub][2] == 0
        assert step[hub][0] != 0 and step[hub][1] != 0
        d_adj, d_cor = _descending(adj, adj.neighbors, hub), _descending(cor, cor.corners, hub)
        step_d = AM.step(V, AM.Adjacency(adj.start, d_adj, adj.boundary, adj.degree), 0.5)
        normals_d = AM.vertex_normals(V, T, cor=AM.Corners(cor.start, d_cor))
        assert not np.array_equal(_u(step_d[hub]), _u(step[hub])), hub
        assert not np.array_equal(_u(normals_d[hub]), _u(normals[hub])), hub
        others = np.arange(nv) != hub
        assert np.array_equal(_u(step_d[others]), _u(step[others])) and np.array_equal(_u(normals_d[others]), _u(normals[others]))


def _descending(csr, items, v):
    """The items of a CSR array with the run of vertex v reversed."""
    out = items.copy()
    a, b = int(csr.start[v]), int(csr.start[v + 1])
    out[a:b] = items[a:b][::-1]
    return out


# ---- the large counts -----------------------------------------------------------------------------------------------------------
def test_loose_triangles_are_more_components_than_65536():
    V, T = SC.loose_triangles()
    assert len(T) == 70000 and len(V) == 210000
    t = TM.topology(V, T)
    assert t.count == 70000 > 65536 and np.all(t.rows[:, :7] == [1, 3, 3, 3, 0, 3, 0]) and np.all(t.rows[:, 7] > 0)
    assert np.array_equal(t.triangle[np.argsort(T.min(axis=1))], np.arange(70000))     # numbered by ascending root: the least vertex
    assert len(np.unique(t.rows[:, 7])) == 5                                           # the rows differ: a row in the wrong place shows


def test_one_big_group():
    V, T = SC.one_big_group()
    for tol in (0.0, 0.5):
        w = WM.weld(V, T, tolerance=tol)
        size = np.bincount(w.rep, minlength=len(V))
        big = int(size.argmax())
        members = np.flatnonzero(w.rep == big)
        assert size[big] > 2 * 2048 and big == members.min() and w.groups > 16
        assert len(set(_u(V[members, 0]).tolist())) >= 2                               # -0.0 and +0.0 in the one group
        assert members.max() - members.min() > 3 * 2048                                # the group straddles tiles
        assert 0 < len(w.vertex_index) < w.groups and 0 < len(w.triangle_index) < len(T)


def test_negative_faces():
    tol = SC.NEGATIVE_FACES_TOLERANCE
    V, T = SC.negative_faces(tol)
    assert len(V) == 66 and len(np.unique(T)) == 66
    rep = WM.weld(V, T, tolerance=tol, flags=3).rep
    for a in range(3):
        for k in SC.FACE_KS:
            on, below, above = (SC.face_vertex(a, k, s) for s in range(3))
            assert V[on, a] == f32(k) * f32(tol) and V[below, a] < V[on, a] < V[above, a]
            assert rep[on] == rep[above] and rep[below] != rep[on], (a, k)
            if k > SC.FACE_KS[0]:
                assert rep[below] == rep[SC.face_vertex(a, k - 1, 0)]
        z = SC.minus_zero_vertex(a)
        assert _u(V[z, a]) == 0x80000000 and rep[z] == rep[SC.face_vertex(a, 0, 0)]
    assert np.any(np.abs(V) < np.finfo(f32).tiny) and np.any(V < 0)


# ---- the wrong variants ---------------------------------------------------------------------------------------------------------
def _census_columns(m, f, inconsistent=None, odd=None):
    cols = [np.ones(len(m), bool), m == 1, m >= 3, m % 2 == 1 if odd is None else odd, (m == 2) & (f != 1) if inconsistent is None else inconsistent]
    return [int(np.sum(c)) for c in cols]


def _topology_variant(**wrong):
    def variant(V, T):
        _, m, f = TM.edges(T)
        want = TM.topology(V, T).census[2:7].tolist()
        assert _census_columns(m, f) == want                                           # (the unchanged lines give the model's census)
        return _census_columns(m, f, **{k: fn(m, f) for k, fn in wrong.items()}), want
    return variant


def test_variant_a_inconsistent_at_every_multiplicity():
    hit = _differs_on(_topology_variant(inconsistent=lambda m, f: f != m - f))
    assert ("book", "even_5000") in hit
    # the same restricted to even multiplicities (at an odd one the two sides can never balance): the subtler mistake
    hit = _differs_on(_topology_variant(inconsistent=lambda m, f: (m % 2 == 0) & (f != m - f)))
    assert ("book", "even_5000") in hit and "archipelago" in hit and ("book", "two_pages") not in hit and ("book", "odd_4999") not in hit


def test_variant_b_odd_means_one():
    hit = _differs_on(_topology_variant(odd=lambda m, f: m == 1))
    assert ("book", "odd_4999") in hit and ("book", "even_5000") not in hit and "archipelago" in hit


def test_variant_c_degenerate_triangles_reference_their_corners():
    def variant(V, T):
        return len(np.unique(T)), int(TM.topology(V, T).census[1])
    hit = _differs_on(variant)
    assert "archipelago" in hit and any(isinstance(n, tuple) and n[0] == "soup" for n in hit)


def test_variant_d_duplicate_triangles_counted_once():
    def variant(V, T):
        _, first = np.unique(np.sort(T, axis=1), axis=0, return_index=True)
        return TM.topology(V, T[np.sort(first)]).census[2:7], TM.topology(V, T).census[2:7]
    hit = _differs_on(variant)
    assert "archipelago" in hit and any(isinstance(n, tuple) and n[0] == "soup" for n in hit)


def _neighbour_records(T):
    L = T[AM.live(T)].astype(i64)
    a, b, c = L[:, 0], L[:, 1], L[:, 2]
    return np.stack([a, b, b, c, c, a], 1).reshape(-1), np.stack([b, a, c, b, a, c], 1).reshape(-1)


def test_variant_e_boundary_means_an_odd_run():
    def variant(V, T):
        frm, to = _neighbour_records(T)
        keys, counts = np.unique(frm << 32 | to, return_counts=True)
        v, w = keys >> 32, keys & 0xFFFFFFFF
        assert np.array_equal(w, AM.adjacency(len(V), T).neighbors)
        boundary = np.zeros(len(V), np.uint8)
        boundary[v[counts % 2 == 1]] = 1
        boundary[w[counts % 2 == 1]] = 1
        return boundary, AM.adjacency(len(V), T).boundary
    hit = _differs_on(variant)
    assert "archipelago" in hit and any(isinstance(n, tuple) and n[0] == "soup" for n in hit)


def test_variant_f_neighbours_not_made_unique():
    def variant(V, T):
        frm, _ = _neighbour_records(T)
        return np.bincount(frm, minlength=len(V)), AM.adjacency(len(V), T).degree
    hit = _differs_on(variant)
    assert ("book", "even_5000") in hit and "archipelago" in hit


# (g) and (h): test_cancelling_book_is_decided_by_the_order_of_the_adds


def _weld_variant(keys_of=None, highest=False):
    def variant(V, T, tol):
        keys = WM.group_keys(V, tol) if keys_of is None else keys_of(V, tol)
        if highest:
            rep, _ = WM.representatives(keys[::-1])
            rep = (len(V) - 1 - rep[::-1]).astype(i32)
        else:
            rep, _ = WM.representatives(keys)
        return rep, WM.weld(V, T, tolerance=tol).rep
    return variant


def _weld_differs_on(variant, tolerances):
    return [(n, tol) for tol in tolerances for n in _cases() if not _equal(*variant(*_cases()[n], tol))]


def test_variant_i_the_highest_index_represents():
    hit = _weld_differs_on(_weld_variant(highest=True), (0.0, 0.25))
    assert ("one_big_group", 0.0) in hit and ("archipelago", 0.25) in hit


def test_variant_j_minus_zero_apart_from_plus_zero():
    hit = _weld_differs_on(_weld_variant(keys_of=lambda V, tol: WM.bits(np.asarray(V, f32).reshape(-1, 3))), (0.0,))
    assert ("one_big_group", 0.0) in hit and ("archipelago", 0.0) in hit and ("negative_faces", 0.0) in hit


def test_variant_k_cells_by_truncation():
    def truncated(V, tol):
        k = np.trunc(np.asarray(V, f32).reshape(-1, 3).astype(f64) / f64(f32(tol)))
        return (k - k.min(axis=0)).astype(i64)
    hit = _weld_differs_on(_weld_variant(keys_of=truncated), (0.25, 0.6))
    assert ("negative_faces", 0.25) in hit and ("archipelago", 0.6) in hit
    assert ("archipelago", 0.25) not in hit          # (multiples of the tolerance: floor and truncation agree; 0.6 is there for this)


def test_variant_l_unreferenced_decided_before_the_weld():
    def variant(V, T, tol):
        w = WM.weld(V, T, tolerance=tol)
        named = np.zeros(len(V), bool)
        named[T[w.triangle_index].reshape(-1)] = True                                  # by the indices as listed, not by representative
        return np.flatnonzero((w.rep == np.arange(len(V))) & named).astype(i32), w.vertex_index
    hit = _weld_differs_on(variant, (0.0, 0.25))
    assert ("one_big_group", 0.0) in hit and ("archipelago", 0.0) in hit
