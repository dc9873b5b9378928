"""Mesh simplification on the MI355X (sdfk_trimesh_simplify and its _device form, csrc/lib_trimesh_simplify.hip) on the stress cases
(tests/mesh_simplify_stress_cases.py; what each case is there for, and which mistake of the library it would show, is proved
from the numpy model alone in tests/test_mesh_simplify_stress_cases.py): centroids and quadrics whose float32 bits the order of
the adds decides, a kept group of 4196 members and a vertex of 3000 corners among 65 535 / 65 537 groups, runs of 4999, 5000
and 5001 equal vertex sets, every byte edge of the group number, triangle counts on both sides of the block and the sort tile
over twelve vertices, fallbacks lane by lane, minimisers exactly on a cell face, an eigenvalue exactly at the truncation, and
coordinates at both ends of the float32 range.  Every case goes through MeshSdf.Simplify and through both entry points into
over-long arrays (the comparisons of tests/test_gpu_mesh_simplify.py, imported from it); everything is compared with the model
as integers and float32 bits, the six stats included -- nothing here has a tolerance."""
import numpy as np
import pytest

from sdfkit_amd.meshsdf import MeshSdf
from tests import mesh_simplify_model as M
from tests import mesh_simplify_stress_cases as S
from tests.test_gpu_mesh_simplify import DUPLICATES, _bits, _check, _same

pytestmark = pytest.mark.gpu
f64 = np.float64
ALL = tuple((p, fl) for p in (0, 1, 2) for fl in (0, 1, 2))


def _sets(T, rep):
    """The vertex sets of the triangles that are not degenerate as groups, and how often each occurs -- counted here, not by the model."""
    G = np.sort(rep[T], axis=1)
    live = ~((G[:, 0] == G[:, 1]) | (G[:, 1] == G[:, 2]))
    _, counts = np.unique(G[live], axis=0, return_counts=True)
    return int(live.sum()), counts


# ---- A, B: the order of the adds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.CENTROID_SIZES)
def test_centroids_decided_by_the_order_of_the_adds(gpu, n):
    V, T, cols, cell = S.centroid_order(n)
    _, out = _check(V, T, cols, cell, ("centroid", n), placements=(1, 2), flag_set=(0,), raw=((1, 0), (2, 0)))
    c = out[1, 0]
    assert c.vertex_index[0] == 0 and np.bincount(c.vertex_map)[0] == n
    assert _bits(c.vertices)[0, 0] == 0x3F000001                                          # the tiny members survived: above the midpoint
    assert _bits(c.vertices)[0, 1] == (0x3F000001 if n > 2 * S.CHUNK else 0x3F000000)      # ... in the second chunk; or were lost at the end


def test_quadrics_on_a_knife_edge(gpu):
    V, T, cols, cell = S.knife_edge()
    _, out = _check(V, T, cols, cell, "knife edge", placements=(2,), flag_set=(0, 1), raw=((2, 0),))
    q = out[2, 0]
    firsts = [i * (S.KNIFE_MEMBERS + 2 * S.KNIFE_CORNERS * S.KNIFE_MEMBERS) for i in range(S.KNIFE_GROUPS)]
    on_face = [bool(q.vertices[q.vertex_map[v], 0] == 4 * i + 1) for i, v in enumerate(firsts)]   # placed: p_x rounds onto the face; fallen back: the centroid
    assert 0 < sum(on_face) < S.KNIFE_GROUPS


def test_triangles_with_two_and_three_corners_in_a_group(gpu):
    V, T, cols, cell = S.shared_corners()
    _, out = _check(V, T, cols, cell, "shared corners", raw=ALL)
    assert out[2, 0].fallbacks == 0


# ---- C: large kept groups -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [65535, 65537])
def test_a_group_of_two_sort_tiles_and_a_hub_of_3000_corners(gpu, groups):
    V, T, cols, cell, (hub, big, mates) = S.large_groups(groups)
    t, out = _check(V, T, cols, cell, ("large", groups), placements=(1, 2), flag_set=(0,), raw=((1, 0), (2, 0)))
    got = t.Simplify(cell, "quadric")
    assert got.Merged == len(V) - groups and got.UnreferencedDropped == groups - (4 + S.HUB_CORNERS) and got.DegenerateDropped == 0
    assert got.DuplicatesDropped == S.BIG_MEMBERS - 1                                       # every member's triangle is the same vertex set
    sizes = np.bincount(got.VertexMap[got.VertexMap >= 0])
    assert sizes[got.VertexMap[big[0]]] == S.BIG_MEMBERS and sizes[got.VertexMap[hub]] == 1 + S.HUB_MATES
    assert np.all(got.VertexMap[big] == got.VertexMap[big[0]]) and np.all(got.VertexMap[mates] == got.VertexMap[hub])


# ---- D: long runs ---------------------------------------------------------------------------------------------------------------
def test_runs_of_equal_vertex_sets_longer_than_two_sort_tiles(gpu):
    V, T, cols, cell, where = S.long_runs()
    t, out = _check(V, T, cols, cell, "long runs", placements=(0, 2), raw=((0, 0), (0, 1), (0, 2)))
    rep = np.arange(len(V))
    rep[26] = 25
    live, counts = _sets(T, rep)
    one, keep, cancel = (t.Simplify(cell, "representative", DUPLICATES[fl]) for fl in (0, 1, 2))
    assert one.DegenerateDropped == keep.DegenerateDropped == cancel.DegenerateDropped == S.DEGENERATE_RUN == len(T) - live
    assert (one.DuplicatesDropped, keep.DuplicatesDropped, cancel.DuplicatesDropped) == (live - len(counts), 0, live - int((counts % 2 == 1).sum()))
    for i, n in enumerate(S.RUNS):
        first, last, count = where[i]
        assert count == n
        copies = np.flatnonzero(np.all(np.sort(T, axis=1) == np.sort(S.RUN_SETS[i]), axis=1))
        kept = np.intersect1d(copies, one.TriangleIndex)
        assert kept.tolist() == [first], (i, kept)                                         # the lowest index of the run, in the middle of the array
        o = int(np.searchsorted(one.TriangleIndex, first))
        assert tuple(one.Triangles[3 * o:3 * o + 3]) == tuple(one.VertexMap[list(S.RUN_SETS[i])])   # with its own winding (a, b, c): no other copy has it
        assert np.intersect1d(copies, cancel.TriangleIndex).tolist() == ([first] if n % 2 else [])
        assert len(np.intersect1d(copies, keep.TriangleIndex)) == n


# ---- E, F: the bytes of the group number; triangle counts -----------------------------------------------------------------------
@pytest.mark.parametrize("groups", S.BYTE_EDGES)
def test_group_counts_at_the_byte_edges(gpu, groups):
    V, T, cols, cell = S.byte_edge(groups)
    t, out = _check(V, T, cols, cell, ("bytes", groups), placements=(0, 2), flag_set=(0, 2), raw=((0, 0), (2, 2)))
    got = t.Simplify(cell, "representative")
    nb = M.index_bytes(groups)
    assert got.Merged == len(V) - groups and got.Passes == out[0, 0].passes == M.W.passes(V, cell) + 3 * nb
    if groups == 2:
        assert len(got.Vertices) == 0 and len(got.Triangles) == 0 and got.DegenerateDropped == len(T)
    else:
        live, counts = _sets(T, np.arange(len(V)))
        assert got.DuplicatesDropped == live - len(counts) and len(got.Triangles) == 3 * len(counts)


@pytest.mark.parametrize("nt", S.TRIANGLE_COUNTS)
def test_triangle_counts_over_twelve_vertices(gpu, nt):
    V, T, cols, cell = S.many_triangles(nt)
    _check(V, T, cols, cell, ("triangles", nt), placements=(0, 2), raw=((2, 0), (2, 2)))


# ---- G: the fallback census -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kept", list(S.SHEET_TILES))
def test_every_group_of_the_tiled_sheets_falls_back(gpu, kept):
    V, T, cols, cell = S.tiled_sheets(kept)
    t, out = _check(V, T, cols, cell, ("sheets", kept), placements=(1, 2), flag_set=(0, 2), raw=((2, 0), (2, 2)))
    got = t.Simplify(cell, "quadric")
    assert got.QuadricFallbacks == out[2, 0].fallbacks == kept == len(got.Vertices)
    assert np.array_equal(_bits(got.Vertices), _bits(t.Simplify(cell, "centroid").Vertices))
    none = t.Simplify(cell, "quadric", "cancel")
    assert none.QuadricFallbacks == 0 and len(none.Vertices) == 0                        # groups that are not kept are not counted


@pytest.mark.parametrize("pattern", list(S.LANE_PATTERNS))
def test_one_fallback_per_wave(gpu, pattern):
    V, T, cols, cell = S.one_per_wave(pattern)
    t, out = _check(V, T, cols, cell, ("wave", pattern), placements=(2,), flag_set=(0, 1), raw=((2, 0),))
    assert t.Simplify(cell, "quadric").QuadricFallbacks == out[2, 0].fallbacks == len(S.LANE_PATTERNS[pattern])


def test_census_of_exact_decisions(gpu):
    V, T, cols, cell, at = S.census()
    t, out = _check(V, T, cols, cell, "census", raw=ALL)
    got = t.Simplify(cell, "quadric")
    assert got.QuadricFallbacks == out[2, 0].fallbacks == len(S.CENSUS_FALLBACKS)
    row = lambda name: (got.Vertices[got.VertexMap[at[name][0]]].astype(f64) / S.U).tolist()   # noqa: E731
    assert row("low_face") == [40.0, 2.0, 2.0]                                                # ON the lower face: placed there
    assert row("high_face") == [82.125, 1.875, 2.0]                                           # ON the upper face: the centroid
    assert row("cut_exact") == [121.0, 1.0, 2.0] and row("cut_above") == [161.0, 1.0, 1.0]    # l == 1e-3 l_max takes no part; an ulp above does
    assert row("l0_small") == [201.0, 1.0, 1.0] and row("zero_area") == [1.0, 1.0, 1.0]
    assert np.all(got.VertexMap[at["unkept"][:2]] == -1)


# ---- H: magnitudes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.SCALES))
def test_coordinates_at_the_ends_of_the_float32_range(gpu, name):
    V, T, cols, cell = S.scaled_corner(name)
    _, out = _check(V, T, cols, cell, ("scaled", name), raw=((1, 0), (2, 0)))
    assert out[2, 0].fallbacks == 0 and np.all(np.isfinite(out[2, 0].vertices)) and np.any(out[2, 0].vertices != 0)


# ---- the order of the calls -----------------------------------------------------------------------------------------------------
def test_quadric_then_centroid_then_quadric_on_one_handle(gpu):
    """The adjacency is built by the first quadric call and reused by the third; nothing else may persist on the handle."""
    for V, T, cols, cell in (S.knife_edge(), S.centroid_order(2 * S.CHUNK + 1), S.census()[:4]):
        t = MeshSdf((V, T) if cols is None else (V, T, cols))
        first, between, again = t.Simplify(cell, "quadric"), t.Simplify(cell, "centroid"), t.Simplify(cell, "quadric")
        _same(first, M.simplify(V, T, cols, cell, 2, 0), "first")
        _same(between, M.simplify(V, T, cols, cell, 1, 0), "between")
        for a, b in ((first.VertexMap, again.VertexMap), (first.VertexIndex, again.VertexIndex), (first.TriangleIndex, again.TriangleIndex),
                     (first.Triangles, again.Triangles), (_bits(first.Vertices), _bits(again.Vertices)), (_bits(first.Colors), _bits(again.Colors))):
            assert np.array_equal(a, b)
        assert [getattr(first, k) == getattr(again, k) for k in ("Merged", "DegenerateDropped", "DuplicatesDropped", "UnreferencedDropped", "Passes",
                                                                  "QuadricFallbacks")] == [True] * 6
