"""Mesh simplification on the MI355X (sdfk_trimesh_simplify and its _device form, csrc/lib_trimesh_simplify.hip) against the numpy
model (tests/mesh_simplify_model.py).  Every output is one stated function of the input, so everything is compared as bits or
integers: hand-made shapes (a flat patch, a crease, a corner: rank 1, 2, 3; two sheets whose minimiser leaves every cell), vertex
counts on both sides of the 256-lane block, the 2048-value scan block and the 2048-record sort tile, a permuted soup whose groups
straddle tiles, groups of 1, 2, kChunk - 1, kChunk, kChunk + 1 and 2 kChunk + 1 members, one group of more than two sort tiles,
duplicate sets of 2, 3 and 4 triangles at the first and last index and across a tile under the three rules, colours present and
absent, cell faces at zero and below, a mesh far from the origin, the weld it equals, and a marching-cubes sphere end to end with
its recorded accuracy."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import MeshSdf
from tests import mesh_simplify_cases as Cs
from tests import mesh_simplify_model as M

pytestmark = pytest.mark.gpu
f32, f64, i32, i64, u32, u8 = np.float32, np.float64, np.int32, np.int64, np.uint32, np.uint8
PLACEMENT = {0: "representative", 1: "centroid", 2: "quadric"}
DUPLICATES = {0: "one", 1: "keep", 2: "cancel"}
ACCURACY = os.path.join(Cs.ROOT, "tests", "golden", "mesh_simplify_accuracy.json")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _stats(want):
    return [want.merged, want.degenerate, want.duplicates, want.unreferenced, want.passes, want.fallbacks]


def _same(got, want, what):
    """A MeshSimplify against the model's Simplify."""
    for g, w, dt in ((got.VertexMap, want.vertex_map, i32), (got.VertexIndex, want.vertex_index, i32), (got.TriangleIndex, want.triangle_index, i32),
                     (got.Triangles, want.triangles, i32)):
        assert g.dtype == dt and np.array_equal(g, w), what
    assert got.Vertices.dtype == f32 and np.array_equal(_bits(got.Vertices), _bits(want.vertices)), what
    assert got.Colors.dtype == f32 and np.array_equal(_bits(got.Colors), _bits(want.colors)), what
    assert [got.Merged, got.DegenerateDropped, got.DuplicatesDropped, got.UnreferencedDropped, got.Passes, got.QuadricFallbacks] == _stats(want), what


def _raw(t, nv, nt, cell, placement, flags, device):
    """Both entry points into arrays one row longer than needed, filled with 7: -> (arrays, kv, kt, stats); the arrays keep their
    7s beyond the counts."""
    L = N.lib()
    kv, kt, st = C.c_int64(-1), C.c_int64(-1), (C.c_int64 * 6)()
    shapes = ((nv + 1,), (nv + 1,), (nt + 1,), (3 * nt + 3,), (nv + 1, 3), (nv + 1, 3))
    if device:
        import torch
        N.bind_torch_stream()
        dev = torch.device("cuda", N._inited_device or 0)
        bufs = [torch.full(s, 7, dtype=torch.int32 if k < 4 else torch.float32, device=dev) for k, s in enumerate(shapes)]
        torch.cuda.synchronize()
        N.check(L.sdfk_trimesh_simplify_device(t.handle, C.c_float(cell), placement, flags, *[C.c_void_p(b.data_ptr()) for b in bufs], C.byref(kv),
                                               C.byref(kt), st))
        out = [b.cpu().numpy() for b in bufs]
    else:
        out = [np.full(s, 7, i32 if k < 4 else f32) for k, s in enumerate(shapes)]
        N.check(L.sdfk_trimesh_simplify(t.handle, C.c_float(cell), placement, flags, *[_vp(a) for a in out], C.byref(kv), C.byref(kt), st))
    return out, kv.value, kt.value, [int(x) for x in st]


def _check_raw(t, nv, nt, cell, placement, flags, want, what):
    for device in (False, True):
        (vm, vi, ti, tr, vs, cs), kv, kt, st = _raw(t, nv, nt, cell, placement, flags, device)
        assert (kv, kt) == (len(want.vertex_index), len(want.triangle_index)), (what, device)
        assert st == _stats(want), (what, device)
        assert np.array_equal(vm[:nv], want.vertex_map) and vm[nv] == 7, (what, device)
        assert np.array_equal(vi[:kv], want.vertex_index) and np.all(vi[kv:] == 7), (what, device)
        assert np.array_equal(ti[:kt], want.triangle_index) and np.all(ti[kt:] == 7), (what, device)
        assert np.array_equal(tr[:3 * kt], want.triangles) and np.all(tr[3 * kt:] == 7), (what, device)
        assert np.array_equal(_bits(vs[:kv]), _bits(want.vertices)) and np.all(vs[kv:] == 7), (what, device)
        assert np.array_equal(_bits(cs[:kv]), _bits(want.colors)) and np.all(cs[kv:] == 7), (what, device)


def _check(V, T, cols, cell, what, placements=Cs.PLACEMENTS, flag_set=Cs.FLAGS, raw=((2, 0),)):
    """Every placement under every duplicate rule through MeshSdf.Simplify, and the (placement, flags) pairs of `raw` through
    both entry points into over-long arrays.  One handle serves them all (the adjacency it builds on the way is its own)."""
    t = MeshSdf((V, T) if cols is None else (V, T, cols))
    out = {}
    for placement in placements:
        for flags in flag_set:
            want = out[placement, flags] = M.simplify(V, T, cols, cell, placement, flags)
            _same(t.Simplify(cell, PLACEMENT[placement], DUPLICATES[flags]), want, (what, placement, flags))
            if (placement, flags) in raw:
                _check_raw(t, len(V), len(T), cell, placement, flags, want, (what, placement, flags))
    return t, out


# ---- the hand-made shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.SMALL))
def test_small_shapes(gpu, name):
    V, T, cols, cell = Cs.SMALL[name]()
    every = [(p, f) for p in Cs.PLACEMENTS for f in Cs.FLAGS]
    _, out = _check(V, T, cols, cell, name, raw=every if name in ("torus_colored", "two_sheets") else ((2, 0),))
    q = out[2, 0]
    if name == "tetrahedron_apart":   # nothing shares a cell: the identity under placements 0 and 1, bit for bit
        for p in (0, 1):
            assert np.array_equal(out[p, 0].vertex_map, np.arange(4)) and np.array_equal(_bits(out[p, 0].vertices), _bits(V))
        assert np.array_equal(q.triangles.reshape(-1, 3), T)
    if name == "flat_patch":          # rank 1: the truncation decides, and nothing falls back
        assert q.fallbacks == 0 and np.allclose(q.vertices[:, 2], 0.25 * q.vertices[:, 0] + 0.125, atol=1e-6)
    if name == "crease":              # rank 2: the cells of the crease are put on its line
        on = (out[1, 0].vertices[:, 0] >= 1.0) & (out[1, 0].vertices[:, 0] < 2.0)
        assert q.fallbacks == 0 and on.sum() == 3 and np.allclose(q.vertices[on, 0], 1.5, atol=1e-6) and np.allclose(q.vertices[on, 2], 0.0, atol=1e-6)
    if name in ("corner", "corner_moved"):   # rank 3: the corner cells are put on the corners, near the origin and far from it
        lo, hi = (f32(0.1), f32(2.35)) if name == "corner" else (f32(0.1) + Cs.MOVED, f32(2.35) + Cs.MOVED)
        tol = 1e-5 if name == "corner" else 2e-3
        assert q.fallbacks == 0 and np.all(np.isclose(q.vertices, lo, rtol=0, atol=tol) | np.isclose(q.vertices, hi, rtol=0, atol=tol), axis=1).sum() == 8
    if name == "two_sheets":          # the minimiser leaves every cell: constructed on the CPU first, non-zero there
        assert q.fallbacks == len(q.vertex_index) == 9 and np.array_equal(_bits(q.vertices), _bits(out[1, 0].vertices))
        assert len(out[2, 2].triangle_index) == 0 and out[2, 2].fallbacks == 0   # sheet on sheet: everything cancels, nothing is placed
    if name == "group_sizes":
        assert sorted(np.bincount(q.vertex_map).tolist()) == [1, 2, Cs.CHUNK - 1, Cs.CHUNK, Cs.CHUNK + 1, 2 * Cs.CHUNK + 1]
    if name == "torus_negative_faces":   # cell faces at zero and below it
        assert V.min() < -2 and np.any(q.cell_index < 0) and np.any(q.cell_index == 0)
    if name == "jittered_soup":
        assert cols is not None and not np.array_equal(_bits(out[1, 0].colors), _bits(out[0, 0].colors))    # the mean of a group's colours, not one of them
    if name == "flat_patch":
        assert cols is None and not np.any(q.colors)


@pytest.mark.parametrize("nv", Cs.SIZES)
def test_block_scan_and_tile_edges(gpu, nv):
    """nv on both sides of 256 (a block of lanes) and of 2048 (a block of the scan, a tile of the sort)."""
    V, T = Cs.sized(nv)
    assert len(V) == nv
    _, out = _check(V, T, None, 0.6, ("sized", nv), placements=(1, 2), flag_set=(0, 2))
    assert out[2, 0].merged > nv // 4
    P, S = Cs.permuted(V, T, nv)
    _check(P, S, Cs.index_colors(nv), 0.6, ("sized permuted", nv), placements=(2,), flag_set=(0,))


def test_permuted_soup_whose_groups_straddle_tiles(gpu):
    V, T = Cs.WC.big_permuted_soup()
    assert len(V) == 3 * 2049
    _, out = _check(V, T, Cs.index_colors(len(V)), 0.3, "big soup", placements=(1, 2), flag_set=(0, 1))
    tile = out[2, 0].rep // Cs.TILE
    assert np.any(tile != np.arange(len(V)) // Cs.TILE)   # members of a group in another tile than their representative


def test_one_group_of_more_than_two_sort_tiles_simplifies_to_nothing(gpu):
    V, T = Cs.one_cell()
    assert len(V) > 2 * Cs.TILE
    _, out = _check(V, T, None, 1.0, "one cell", raw=((2, 0), (0, 1)))
    for s in out.values():
        assert (len(s.vertex_index), len(s.triangle_index), s.merged, s.unreferenced) == (0, 0, len(V) - 1, 1) and np.all(s.vertex_map == -1)


def test_duplicate_sets_at_the_first_and_last_index_and_across_a_tile(gpu):
    V, T = Cs.duplicate_sets()
    nt = len(T)
    assert nt > Cs.TILE
    _, out = _check(V, T, None, 0.2, "duplicate sets", placements=(0, 2), raw=((0, 0), (0, 1), (0, 2)))
    gone = lambda s: sorted(set(range(nt)) - set(s.triangle_index.tolist()))   # noqa: E731
    assert gone(out[0, 0]) == [8, Cs.TILE - 1, Cs.TILE, nt - 3, nt - 2, nt - 1] and gone(out[0, 1]) == []
    assert gone(out[0, 2]) == [0, 8, 10, Cs.TILE - 1, Cs.TILE, nt - 3, nt - 2, nt - 1]
    assert [out[0, f].duplicates for f in Cs.FLAGS] == [6, 0, 8]


def test_placement_0_keeping_duplicates_is_the_weld_on_the_device(gpu):
    for name in ("fine_torus", "jittered_soup", "thin_slab"):
        V, T, cols, cell = Cs.SMALL[name]()
        t = MeshSdf((V, T) if cols is None else (V, T, cols))
        s, w = t.Simplify(cell, "representative", "keep"), t.Weld(cell)
        for a, b in ((s.VertexMap, w.VertexMap), (s.VertexIndex, w.VertexIndex), (s.TriangleIndex, w.TriangleIndex), (s.Triangles, w.Triangles),
                     (_bits(s.Vertices), _bits(w.Vertices)), (_bits(s.Colors), _bits(w.Colors))):
            assert np.array_equal(a, b), name
        assert (s.Merged, s.DegenerateDropped, s.UnreferencedDropped, s.Passes, s.DuplicatesDropped, s.QuadricFallbacks) == \
            (w.Merged, w.DegenerateDropped, w.UnreferencedDropped, w.Passes, 0, 0), name
        # simplifying twice with placement 0 changes nothing the second time
        first = t.Simplify(cell, "representative")
        again = MeshSdf((first.Vertices, first.Triangles) if cols is None else (first.Vertices, first.Triangles, first.Colors)).Simplify(cell, "representative")
        assert np.array_equal(again.VertexMap, np.arange(len(first.Vertices))) and np.array_equal(again.Triangles, first.Triangles), name
        assert np.array_equal(_bits(again.Vertices), _bits(first.Vertices)) and np.array_equal(_bits(again.Colors), _bits(first.Colors)), name


def test_null_outputs_one_at_a_time_and_an_unchanged_handle(gpu):
    V, T, cols, cell = Cs.SMALL["torus_colored"]()
    t = MeshSdf((V, T, cols))
    want = M.simplify(V, T, cols, cell, 2, 0)
    nv, nt, L = len(V), len(T), N.lib()
    q = np.array([[0.1, 0.2, 0.3], [2.0, -1.0, 0.5]], f32)
    before = t.Search(q)
    for skip in range(9):
        arrays = [np.full(s, 7, i32 if k < 4 else f32) for k, s in enumerate(((nv,), (nv,), (nt,), (3 * nt,), (nv, 3), (nv, 3)))]
        kv, kt, st = C.c_int64(-1), C.c_int64(-1), (C.c_int64 * 6)()
        ptrs = [_vp(a) for a in arrays] + [C.byref(kv), C.byref(kt), st]
        ptrs[skip] = None
        N.check(L.sdfk_trimesh_simplify(t.handle, C.c_float(cell), 2, 0, *ptrs))
        vm, vi, ti, tr, vs, cs = arrays
        k, m = len(want.vertex_index), len(want.triangle_index)
        checks = [lambda: np.array_equal(vm, want.vertex_map), lambda: np.array_equal(vi[:k], want.vertex_index),
                  lambda: np.array_equal(ti[:m], want.triangle_index), lambda: np.array_equal(tr[:3 * m], want.triangles),
                  lambda: np.array_equal(_bits(vs[:k]), _bits(want.vertices)), lambda: np.array_equal(_bits(cs[:k]), _bits(want.colors)),
                  lambda: kv.value == k, lambda: kt.value == m, lambda: list(st) == _stats(want)]
        for j, ok in enumerate(checks):
            if j != skip:
                assert ok(), (skip, j)
        if skip < 6:
            assert np.all(arrays[skip] == 7)
    st = (C.c_int64 * 6)()
    N.check(L.sdfk_trimesh_simplify(t.handle, C.c_float(cell), 2, 0, *[None] * 8, st))          # nothing but the stats: the fallbacks are counted all the same
    assert list(st) == _stats(want) and want.fallbacks > 0
    N.check(L.sdfk_trimesh_simplify_device(t.handle, C.c_float(cell), 2, 0, *[None] * 9))
    after = t.Search(q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
    assert t.Topology().Vertices == nv and np.array_equal(t.Weld().Triangles, T.reshape(-1))       # the handle still holds the torus


def test_device_outputs_go_straight_into_a_new_handle(gpu):
    import torch
    N.bind_torch_stream()
    dev = torch.device("cuda", N._inited_device or 0)
    V, T, _, cell = Cs.SMALL["corner"]()
    want = M.simplify(V, T, None, cell, 2, 2)
    t = MeshSdf((V, T))
    tr = torch.zeros(3 * len(T), dtype=torch.int32, device=dev)
    vs = torch.zeros((len(V), 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    kv, kt, st = t.SimplifyDevice(cell, "quadric", "cancel", triangles_dev=tr.data_ptr(), vertices_dev=vs.data_ptr())
    assert (kv, kt, st) == (len(want.vertex_index), len(want.triangle_index), _stats(want))
    h = C.c_void_p()
    L = N.lib()
    N.check(L.sdfk_trimesh_create_device(C.c_void_p(vs.data_ptr()), kv, C.c_void_p(tr.data_ptr()), 3 * kt, None, C.byref(h)))
    try:
        census = (C.c_int64 * 8)()
        N.check(L.sdfk_trimesh_topology(h, census, None, 0))
        assert census[0] == 1 and census[1] == kv and census[5] == 0          # one component, every vertex used, no edge used an odd number of times
    finally:
        L.sdfk_trimesh_free(h)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    V, T = Cs.tetrahedron()
    W3 = np.array([(0, 0, 0), (2 ** 21, 0.5, -3), (1, 1, 1)], f32)       # spans 2^21 + 1 cells of the lattice 1.0 along x
    ok = np.array([(0, 0, 0), (2 ** 21 - 1, 0.5, -3), (1, 1, 1)], f32)
    t, wide, fits = MeshSdf((V, T)), MeshSdf((W3, np.array([0, 1, 2], i32))), MeshSdf((ok, np.array([0, 1, 2], i32)))
    L = N.lib()
    arrays = [np.full(s, 7, i32 if k < 4 else f32) for k, s in enumerate(((4,), (4,), (4,), (12,), (4, 3), (4, 3)))]
    kv, kt, st = C.c_int64(-7), C.c_int64(-7), (C.c_int64 * 6)(*[-7] * 6)
    outs = [_vp(a) for a in arrays] + [C.byref(kv), C.byref(kt), st]
    null, fl = C.c_void_p(), C.c_float
    bad_cell = "cellSize must be finite and greater than 0"
    calls = [("null argument", lambda f: f(null, fl(1.0), 2, 0, *outs)),
             (bad_cell, lambda f: f(t.handle, fl(0.0), 2, 0, *outs)),
             (bad_cell, lambda f: f(t.handle, fl(-1e-3), 2, 0, *outs)),
             (bad_cell, lambda f: f(t.handle, fl(np.nan), 2, 0, *outs)),
             (bad_cell, lambda f: f(t.handle, fl(np.inf), 2, 0, *outs)),
             ("unknown placement", lambda f: f(t.handle, fl(1.0), 3, 0, *outs)),
             ("unknown placement", lambda f: f(t.handle, fl(1.0), -1, 0, *outs)),
             ("unknown flag bits", lambda f: f(t.handle, fl(1.0), 2, 4, *outs)),
             ("unknown flag bits", lambda f: f(t.handle, fl(1.0), 2, -1, *outs)),
             ("exclude each other", lambda f: f(t.handle, fl(1.0), 2, 3, *outs)),
             ("an axis spans 2^21 cells", lambda f: f(wide.handle, fl(1.0), 2, 0, *outs))]
    for message, call in calls:
        for fn in (L.sdfk_trimesh_simplify, L.sdfk_trimesh_simplify_device):   # (refused before any output is touched: host arrays do for both)
            assert call(fn) == N.ERR_INVALID, message
            err = L.sdfk_last_error().decode()
            assert "sdfk_trimesh_simplify" in err and message in err, (message, err)
    assert all(np.all(a == 7) for a in arrays) and kv.value == -7 and kt.value == -7 and list(st) == [-7] * 6
    with pytest.raises(N.SdfKitNativeError):
        wide.Simplify(1.0)
    with pytest.raises(ValueError):
        t.Simplify(1.0, "nearest")
    with pytest.raises(ValueError):
        t.Simplify(1.0, "quadric", "both")
    assert len(fits.Simplify(1.0).Vertices) == 3                                           # one cell fewer: accepted
    assert wide.Simplify(2.0).Merged == 1                                                  # half the cells: (0, 0, 0) and (1, 1, 1) share one
    _same(t.Simplify(0.5), M.simplify(V, T, None, 0.5, 2, 0), "after the refusals")        # (the handle is as usable as before)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
RADIUS, GRID = 0.8, 64
VOXEL = float(f32(2.0 / GRID))            # the volume's voxel: (max - min) / n
# The sphere the MESH lies on: the volume samples cell centres, min + (i + 1/2) (max - min) / n, and ToMesh (as the reference's
# MarchingCubes does) maps grid index i to min + i (max - min) / (n - 1): over a box centred at the origin that is the surface scaled
# by n / (n - 1) about the origin.  The error of a simplification is measured from there (the test asserts that the input is there).
MESH_RADIUS = RADIUS * GRID / (GRID - 1)


@functools.lru_cache(maxsize=None)
def _sphere():
    E = K.SdfExprs
    return E.Sphere(RADIUS, (1.0, 0.4, 0.2)).ToSdf().ToMesh([-1.0] * 3, [1.0] * 3, GRID, GRID, GRID)


@functools.lru_cache(maxsize=None)
def _sphere_arrays():
    m = _sphere()
    return np.array(m.Vertices, f32).reshape(-1, 3), np.array(m.Triangles, i32).reshape(-1, 3), np.array(m.Colors, f32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def _sphere_model(voxels, placement, flags):
    V, T, cols = _sphere_arrays()
    return M.simplify(V, T, cols, f32(voxels * VOXEL), placement, flags)


def rms_radius_error(vertices):
    """sqrt(mean((|v| - r)^2)), r = MESH_RADIUS, in float64 from the float32 vertices; the mean by math.fsum, which does not depend
    on an order."""
    v = np.asarray(vertices, f32).astype(f64)
    e = np.abs(np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) - f64(MESH_RADIUS))
    return math.sqrt(math.fsum((e * e).tolist()) / len(e))


@pytest.mark.parametrize("voxels", [2, 4])
def test_marching_cubes_sphere_through_mesh_simplify(gpu, voxels):
    m = _sphere()
    V, T, cols = _sphere_arrays()
    cell = f32(voxels * VOXEL)
    assert m.Topology().IsWatertight
    for placement in ("centroid", "quadric"):
        want = _sphere_model(voxels, {"centroid": 1, "quadric": 2}[placement], M.CANCEL_PAIRS)
        s = m.Simplify(cell, placement, "cancel")
        assert np.array_equal(_bits(s.Vertices), _bits(want.vertices)) and np.array_equal(s.Triangles, want.triangles)
        assert np.array_equal(_bits(s.Colors), _bits(want.colors))
        assert np.array_equal(s.Min, want.vertices.min(axis=0)) and np.array_equal(s.Max, want.vertices.max(axis=0))
        assert 0 < len(s.Triangles) < len(m.Triangles) and s.Topology().IsWatertight
        grown_lo, grown_hi = V.min(axis=0) - cell, V.max(axis=0) + cell
        assert np.all(s.Vertices >= grown_lo) and np.all(s.Vertices <= grown_hi)
        # normals: from the new geometry on the side of the representatives' gathered ones; or gathered
        g = m.Simplify(cell, placement, "cancel", normals=False)
        assert np.array_equal(_bits(g.Normals), _bits(np.array(m.Normals, f32).reshape(-1, 3)[want.vertex_index]))
        assert np.array_equal(_bits(s.Normals), _bits(g.RecomputeNormals().Normals))
        outward = (s.Normals.astype(f64) * s.Vertices.astype(f64)).sum(axis=1)
        assert np.count_nonzero(outward > 0) > len(outward) // 2          # the sphere's gradient normals point outwards, and the new ones keep the side
    one = m.Simplify(cell)      # the defaults: quadric, one of each set
    want = _sphere_model(voxels, 2, 0)
    assert np.array_equal(_bits(one.Vertices), _bits(want.vertices)) and np.array_equal(one.Triangles, want.triangles)


def test_everything_in_one_cell_gives_an_empty_mesh(gpu):
    V, T, _, _ = Cs.SMALL["flat_patch"]()
    m = K.Mesh(V, np.zeros_like(V), np.zeros_like(V), T.reshape(-1))
    e = m.Simplify(64.0)
    assert len(e.Vertices) == 0 and len(e.Triangles) == 0 and e.Vertices.shape == (0, 3) and e.Normals.shape == (0, 3)


def test_accuracy_on_the_sphere_is_the_recorded_one(gpu):
    """The RMS of | |v| - r | over the output vertices, centroid and quadric at 2, 4 and 8 voxels, recorded from the model in
    tests/golden/mesh_simplify_accuracy.json.  Asserted: centroids of points of a convex surface lie inside it, so the quadric's
    RMS is below the centroid's at every size; and the device reproduces the recorded values exactly.  r is the radius of the
    sphere the input mesh lies on (MESH_RADIUS; the input's own RMS about it is asserted to be below the h^2 / (8 r) of a linear
    crossing, 1.5e-4).  The margin is narrow, 20 % at 2 voxels and 1 % at 8: with all three eigenpairs above the truncation the
    minimiser of a cap's tangent planes lies OUTSIDE the sphere by about as much as the centroid lies inside."""
    with open(ACCURACY) as f:
        doc = json.load(f)
    m = _sphere()
    assert (doc["radius"], doc["grid"], doc["vertices"], doc["triangles"]) == (RADIUS, GRID, len(m.Vertices), len(m.Triangles) // 3)
    assert doc["mesh_radius"] == MESH_RADIUS and doc["input"] == rms_radius_error(m.Vertices) < VOXEL * VOXEL / (8 * RADIUS)
    sdf = MeshSdf(m)
    for voxels in (2, 4, 8):
        row = doc["rms"][str(voxels)]
        got = {}
        for placement in ("centroid", "quadric"):
            s = sdf.Simplify(f32(voxels * VOXEL), placement)
            want = _sphere_model(voxels, {"centroid": 1, "quadric": 2}[placement], 0)
            assert np.array_equal(_bits(s.Vertices), _bits(want.vertices))
            got[placement] = rms_radius_error(s.Vertices)
            assert got[placement] == rms_radius_error(want.vertices) == row[placement], (voxels, placement, got[placement], row[placement])
            assert row[placement + "_vertices"] == len(s.Vertices) and row[placement + "_fallbacks"] == s.QuadricFallbacks
        print(voxels, got)
        assert got["quadric"] < got["centroid"], (voxels, got)
