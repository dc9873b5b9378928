"""Mesh welding on the MI355X (sdfk_trimesh_weld and its _device form, csrc/lib_trimesh_weld.hip) against the numpy model
(tests/mesh_weld_model.py).  Every output is one stated function of the input, so everything is compared as bits or integers.
The meshes are small, tidy ones, no group of more than 6 vertices (a weld group longer than two sort tiles, random index soups
and the lattice's cell faces at zero and below are in tests/test_gpu_mesh_stress.py): soups of hand-made shapes, pairs that
differ in one coordinate (the boundary between the two sorts), -0 against +0, one group, duplicates at the first and last index,
sizes on both sides of the 256-lane block, the 2048-value scan block and the 2048-record sort tile, a permuted soup whose groups
straddle tiles, every flag, colours, far from the origin and at subnormal scale, the lattice mode at cell centres and across a
cell face.  Then a marching-cubes sphere taken apart and welded again."""
import ctypes as C
import functools

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import MeshSdf
from tests import mesh_weld_cases as Cs
from tests import mesh_weld_model as M

pytestmark = pytest.mark.gpu
f32, f64, i32, i64, u32, u8 = np.float32, np.float64, np.int32, np.int64, np.uint32, np.uint8


def _bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _same(got, want, passes, what):
    """A MeshWeld against the model's Weld."""
    for g, w, dt in ((got.VertexMap, want.vertex_map, i32), (got.VertexIndex, want.vertex_index, i32), (got.TriangleIndex, want.triangle_index, i32),
                     (got.Triangles, want.triangles, i32)):
        assert g.dtype == dt and np.array_equal(g, w), what
    assert got.Vertices.dtype == f32 and np.array_equal(_bits(got.Vertices), _bits(want.vertices)), what
    assert got.Colors.dtype == f32 and np.array_equal(_bits(got.Colors), _bits(want.colors)), what
    assert (got.Merged, got.DegenerateDropped, got.UnreferencedDropped, got.Passes) == (want.merged, want.degenerate, want.unreferenced, passes), what


def _raw(t, nv, nt, tol, flags, device):
    """Both entry points into arrays one row longer than needed, filled with 7: -> (arrays, kv, kt, stats); the arrays keep their
    7s beyond the counts."""
    L = N.lib()
    kv, kt, st = C.c_int64(-1), C.c_int64(-1), (C.c_int64 * 4)()
    shapes = ((nv + 1,), (nv + 1,), (nt + 1,), (3 * nt + 3,), (nv + 1, 3), (nv + 1, 3))
    if device:
        import torch
        N.bind_torch_stream()
        dev = torch.device("cuda", N._inited_device or 0)
        bufs = [torch.full(s, 7, dtype=torch.int32 if k < 4 else torch.float32, device=dev) for k, s in enumerate(shapes)]
        torch.cuda.synchronize()
        N.check(L.sdfk_trimesh_weld_device(t.handle, C.c_float(tol), flags, *[C.c_void_p(b.data_ptr()) for b in bufs], C.byref(kv), C.byref(kt), st))
        out = [b.cpu().numpy() for b in bufs]
    else:
        out = [np.full(s, 7, i32 if k < 4 else f32) for k, s in enumerate(shapes)]
        N.check(L.sdfk_trimesh_weld(t.handle, C.c_float(tol), flags, *[_vp(a) for a in out], C.byref(kv), C.byref(kt), st))
    return out, kv.value, kt.value, [int(x) for x in st]


def _check_raw(t, V, T, cols, tol, flags, want, passes, what):
    nv, nt = len(V), len(T)
    for device in (False, True):
        (vm, vi, ti, tr, vs, cs), kv, kt, st = _raw(t, nv, nt, tol, flags, device)
        assert (kv, kt) == (len(want.vertex_index), len(want.triangle_index)), (what, device)
        assert st == [want.merged, want.degenerate, want.unreferenced, passes], (what, device)
        assert np.array_equal(vm[:nv], want.vertex_map) and vm[nv] == 7, (what, device)
        assert np.array_equal(vi[:kv], want.vertex_index) and np.all(vi[kv:] == 7), (what, device)
        assert np.array_equal(ti[:kt], want.triangle_index) and np.all(ti[kt:] == 7), (what, device)
        assert np.array_equal(tr[:3 * kt], want.triangles) and np.all(tr[3 * kt:] == 7), (what, device)
        assert np.array_equal(_bits(vs[:kv]), _bits(want.vertices)) and np.all(vs[kv:] == 7), (what, device)
        assert np.array_equal(_bits(cs[:kv]), _bits(want.colors)) and np.all(cs[kv:] == 7), (what, device)


def _check(V, T, cols, tol, what, flag_set=Cs.FLAGS, raw_flags=(0,)):
    t = MeshSdf((V, T) if cols is None else (V, T, cols))
    passes = M.passes(V, tol)
    out = {}
    for flags in flag_set:
        want = out[flags] = M.weld(V, T, cols, tol, flags)
        _same(t.Weld(tol, bool(flags & 1), bool(flags & 2)), want, passes, (what, flags))
        if flags in raw_flags:
            _check_raw(t, V, T, cols, tol, flags, want, passes, (what, flags))
    return t, out


# ---- the small shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.SMALL))
def test_small_shapes(gpu, name):
    V, T, cols, tol = Cs.SMALL[name]()
    t, out = _check(V, T, cols, tol, name, raw_flags=Cs.FLAGS if name == "unreferenced_and_degenerate" else (0,))
    w = out[0]
    if name == "tetrahedron_soup":
        assert len(w.vertex_index) == 4 and w.merged == 8
    if name == "tetrahedron_clean":   # the identity, bit for bit
        assert np.array_equal(w.vertex_map, np.arange(4)) and np.array_equal(w.triangles.reshape(-1, 3), T) and np.array_equal(_bits(w.vertices), _bits(V))
    if name == "all_equal":
        assert (len(w.vertex_index), len(w.triangle_index)) == (0, 0) and np.all(w.vertex_map == -1)
        assert len(out[3].vertex_index) == 1 and len(out[3].triangle_index) == 2
    if name == "signed_zeros":
        assert w.rep.tolist() == [0, 1, 2, 0, 1, 2, 6] and np.array_equal(_bits(t.Weld().Vertices[0]), _bits(V[0]))
    if name == "torus_soup_colored":
        assert np.array_equal(_bits(w.colors), _bits(cols[w.vertex_index])) and np.any(cols != cols[w.rep])   # the twins' colours differ
    if name == "straddling_pair_lattice":
        assert len(w.vertex_index) == 4 and w.vertex_map[0] != w.vertex_map[1]
    if name == "jittered_lattice":
        assert len(w.vertex_index) == 48 and len(M.weld(V, T).vertex_index) == len(V)   # as values they all differ
    if name == "strip_soup_tiny":
        assert np.all(np.abs(V) < np.finfo(f32).tiny) and len(w.vertex_index) == 40


@pytest.mark.parametrize("nv", Cs.SIZES)
def test_block_scan_and_tile_edges(gpu, nv):
    """nv on both sides of 256 (a block of lanes) and of 2048 (a block of the scan, a tile of the sort), exact and lattice."""
    V, T = Cs.sized(nv)
    assert len(V) == nv
    _, out = _check(V, T, None, 0.0, ("sized", nv), flag_set=(0, 3))
    assert out[0].merged == 40
    W, S = Cs.permuted(V, T, nv)
    _check(W, S, Cs.index_colors(nv), 0.0, ("sized permuted", nv), flag_set=(0,))
    _check(W, S, None, 0.05, ("sized permuted lattice", nv), flag_set=(0,))


def test_permuted_soup_whose_groups_straddle_tiles(gpu):
    V, T = Cs.big_permuted_soup()
    assert len(V) == 3 * 2049
    _, out = _check(V, T, Cs.index_colors(len(V)), 0.0, "big soup", flag_set=(0, 1))
    assert len(out[0].vertex_index) == 2051 and out[0].degenerate == 0
    tile = out[0].rep // 2048
    assert np.any(tile != np.arange(len(V)) // 2048)   # members of a group in another tile than their representative
    _, lat = _check(V, T, None, 0.5, "big soup lattice", flag_set=(0,), raw_flags=())
    assert 0 < len(lat[0].vertex_index) < 2051        # a lattice coarser than the strip merges neighbours too


def test_welding_a_welded_mesh_is_the_identity(gpu):
    for name in ("cube_soup", "unreferenced_and_degenerate", "jittered_lattice"):
        V, T, cols, tol = Cs.SMALL[name]()
        first = MeshSdf((V, T) if cols is None else (V, T, cols)).Weld(tol)
        again = MeshSdf((first.Vertices, first.Triangles) if cols is None else (first.Vertices, first.Triangles, first.Colors)).Weld(tol)
        assert np.array_equal(again.VertexMap, np.arange(len(first.Vertices))) and np.array_equal(again.Triangles, first.Triangles)
        assert np.array_equal(_bits(again.Vertices), _bits(first.Vertices)) and np.array_equal(_bits(again.Colors), _bits(first.Colors))
        assert (again.Merged, again.DegenerateDropped, again.UnreferencedDropped) == (0, 0, 0)


def test_null_outputs_one_at_a_time_and_an_unchanged_handle(gpu):
    V, T, cols, tol = Cs.SMALL["torus_soup_colored"]()
    t = MeshSdf((V, T, cols))
    want = M.weld(V, T, cols, tol)
    nv, nt, L = len(V), len(T), N.lib()
    q = np.array([[0.1, 0.2, 0.3], [2.0, -1.0, 0.5]], f32)
    before = t.Search(q)
    for skip in range(9):
        arrays = [np.full(s, 7, i32 if k < 4 else f32) for k, s in enumerate(((nv,), (nv,), (nt,), (3 * nt,), (nv, 3), (nv, 3)))]
        kv, kt, st = C.c_int64(-1), C.c_int64(-1), (C.c_int64 * 4)()
        ptrs = [_vp(a) for a in arrays] + [C.byref(kv), C.byref(kt), st]
        ptrs[skip] = None
        N.check(L.sdfk_trimesh_weld(t.handle, C.c_float(tol), 0, *ptrs))
        vm, vi, ti, tr, vs, cs = arrays
        k, m = len(want.vertex_index), len(want.triangle_index)
        checks = [lambda: np.array_equal(vm, want.vertex_map), lambda: np.array_equal(vi[:k], want.vertex_index),
                  lambda: np.array_equal(ti[:m], want.triangle_index), lambda: np.array_equal(tr[:3 * m], want.triangles),
                  lambda: np.array_equal(_bits(vs[:k]), _bits(want.vertices)), lambda: np.array_equal(_bits(cs[:k]), _bits(want.colors)),
                  lambda: kv.value == k, lambda: kt.value == m, lambda: list(st)[:3] == [want.merged, want.degenerate, want.unreferenced]]
        for j, ok in enumerate(checks):
            if j != skip:
                assert ok(), (skip, j)
        if skip < 6:
            assert np.all(arrays[skip] == 7)
    N.check(L.sdfk_trimesh_weld(t.handle, C.c_float(tol), 0, *[None] * 9))          # nothing asked for: still not an error
    N.check(L.sdfk_trimesh_weld_device(t.handle, C.c_float(tol), 0, *[None] * 9))
    after = t.Search(q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
    assert t.Topology().Components == len(T)                                          # the handle still holds the soup


def test_device_outputs_go_straight_into_a_new_handle(gpu):
    import torch
    N.bind_torch_stream()
    dev = torch.device("cuda", N._inited_device or 0)
    V, T, _, _ = Cs.SMALL["cube_soup"]()
    t = MeshSdf((V, T))
    tr = torch.zeros(3 * len(T), dtype=torch.int32, device=dev)
    vs = torch.zeros((len(V), 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    kv, kt, st = t.WeldDevice(0.0, False, False, triangles_dev=tr.data_ptr(), vertices_dev=vs.data_ptr())
    assert (kv, kt, st[:3]) == (8, 12, [28, 0, 0])
    h = C.c_void_p()
    L = N.lib()
    N.check(L.sdfk_trimesh_create_device(C.c_void_p(vs.data_ptr()), kv, C.c_void_p(tr.data_ptr()), 3 * kt, None, C.byref(h)))
    try:
        census = (C.c_int64 * 8)()
        N.check(L.sdfk_trimesh_topology(h, census, None, 0))
        assert list(census) == [1, 8, 18, 0, 0, 0, 0, 0]
    finally:
        L.sdfk_trimesh_free(h)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    V, T = Cs.soup(*Cs.tetrahedron())
    W = np.array([(0, 0, 0), (2 ** 21, 0.5, -3), (1, 1, 1)], f32)       # spans 2^21 + 1 cells of the lattice 1.0 along x
    ok = np.array([(0, 0, 0), (2 ** 21 - 1, 0.5, -3), (1, 1, 1)], f32)
    t, wide, fits = MeshSdf((V, T)), MeshSdf((W, np.array([0, 1, 2], i32))), MeshSdf((ok, np.array([0, 1, 2], i32)))
    L = N.lib()
    arrays = [np.full(s, 7, i32 if k < 4 else f32) for k, s in enumerate(((12,), (12,), (4,), (12,), (12, 3), (12, 3)))]
    kv, kt, st = C.c_int64(-7), C.c_int64(-7), (C.c_int64 * 4)(-7, -7, -7, -7)
    outs = [_vp(a) for a in arrays] + [C.byref(kv), C.byref(kt), st]
    null, fl = C.c_void_p(), C.c_float
    calls = [("null argument", lambda f: f(null, fl(0.0), 0, *outs)),
             ("tolerance must be finite and not negative", lambda f: f(t.handle, fl(-1e-3), 0, *outs)),
             ("tolerance must be finite and not negative", lambda f: f(t.handle, fl(np.nan), 0, *outs)),
             ("tolerance must be finite and not negative", lambda f: f(t.handle, fl(np.inf), 0, *outs)),
             ("unknown flag bits", lambda f: f(t.handle, fl(0.0), 4, *outs)),
             ("unknown flag bits", lambda f: f(t.handle, fl(0.0), -1, *outs)),
             ("an axis spans 2^21 cells", lambda f: f(wide.handle, fl(1.0), 0, *outs))]
    for message, call in calls:
        for fn in (L.sdfk_trimesh_weld, L.sdfk_trimesh_weld_device):   # (refused before any output is touched: host arrays do for both)
            assert call(fn) == N.ERR_INVALID, message
            err = L.sdfk_last_error().decode()
            assert "sdfk_trimesh_weld" in err and message in err, (message, err)
    assert all(np.all(a == 7) for a in arrays) and kv.value == -7 and kt.value == -7 and list(st) == [-7] * 4
    with pytest.raises(N.SdfKitNativeError):
        wide.Weld(1.0)
    assert len(fits.Weld(1.0).Vertices) == 3 and len(wide.Weld(0.0).Vertices) == 3      # one cell fewer, and exact mode: no span
    assert wide.Weld(2.0).Merged == 1                                                     # half the cells: accepted ((0, 0, 0) and (1, 1, 1) share one)
    _same(t.Weld(), M.weld(V, T), M.passes(V, 0.0), "after the refusals")   # (the handle is as usable as before)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere():
    """A radius at which the indexed mesh has no two equal positions (checked below with the model)."""
    E = K.SdfExprs
    return E.Sphere(0.8, (1.0, 0.4, 0.2)).ToSdf().ToMesh([-1.0] * 3, [1.0] * 3, 24, 24, 24)


def _soup_mesh(m):
    T = np.array(m.Triangles, i32).reshape(-1)
    g = lambda a: np.ascontiguousarray(np.array(a, f32).reshape(-1, 3)[T])   # noqa: E731
    return K.Mesh(g(m.Vertices), g(m.Colors), g(m.Normals), np.arange(len(T), dtype=i32), np.array(m.Min, f32), np.array(m.Max, f32))


def test_a_soup_gets_its_connectivity_back(gpu):
    m = _sphere()
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, i32).reshape(-1, 3)
    nv, nt = len(V), len(T)
    clean = M.weld(V, T)
    assert nv > 500 and (clean.merged, clean.degenerate, clean.unreferenced) == (0, 0, 0)
    s = _soup_mesh(m)
    before = s.Topology()
    assert before.Components == nt and not before.IsWatertight
    w = s.Weld()
    want = M.weld(s.Vertices, s.Triangles, s.Colors)
    assert len(w.Vertices) == nv and len(w.Triangles) == 3 * nt
    assert np.array_equal(_bits(w.Vertices), _bits(want.vertices)) and np.array_equal(w.Triangles, want.triangles)
    assert np.array_equal(_bits(w.Colors), _bits(want.colors)) and np.array_equal(_bits(w.Normals), _bits(s.Normals[want.vertex_index]))
    assert np.array_equal(w.Min, want.vertices.min(axis=0)) and np.array_equal(w.Max, want.vertices.max(axis=0))
    assert np.array_equal(_bits(w.Vertices[w.Triangles]), _bits(V[T.reshape(-1)]))       # every triangle where it was
    topo = w.Topology()
    assert w.Components().Count == 1 and topo.Components == 1
    assert topo.IsWatertight and topo.IsOriented and topo.EulerCharacteristic == 2
    box = ([-1.0] * 3, [1.0] * 3, 20, 20, 20)
    a, b = w.ToVoxels(*box), m.ToVoxels(*box)
    assert np.array_equal(_bits(a.Values), _bits(b.Values))
    moved = w.Smooth(1)
    assert not np.array_equal(_bits(moved.Vertices), _bits(w.Vertices))
    assert np.array_equal(_bits(s.Smooth(1).Vertices), _bits(s.Vertices))                 # the soup: nothing pulls on anything
    # normals from the welded geometry, on the side of the gathered ones
    r = s.Weld(normals=True)
    assert np.array_equal(_bits(r.Normals), _bits(w.RecomputeNormals().Normals)) and not np.array_equal(_bits(r.Normals), _bits(w.Normals))
    assert np.all((r.Normals.astype(f64) * w.Normals.astype(f64)).sum(axis=1) > 0.9)
    # the lattice mode with a cell far below the mesh's spacing does the same
    assert len(s.Weld(1e-4).Vertices) == nv


def test_concat_then_weld(gpu):
    m = _sphere()
    far = K.Mesh(np.array(m.Vertices, f32) + np.array([4, 0, 0], f32), m.Colors, m.Normals, m.Triangles)
    both = K.Mesh.Concat([_soup_mesh(m), _soup_mesh(far)])
    nt = len(m.Triangles) // 3
    assert len(both.Vertices) == 6 * nt and both.Triangles.dtype == i32 and both.Topology().Components == 2 * nt
    assert np.array_equal(both.Min, np.array(m.Vertices, f32).min(axis=0)) and np.array_equal(both.Max, far.Vertices.max(axis=0))
    w = both.Weld()
    c = w.Components()
    assert c.Count == 2 and len(w.Vertices) == 2 * len(m.Vertices) and c.Triangles.tolist() == [nt, nt]
    assert np.all(c.IsWatertight) and c.EulerCharacteristic.tolist() == [2, 2]
    # two copies in one place weld into one doubled surface: one component, every edge used four times
    twice = K.Mesh.Concat([m, m]).Weld()
    assert len(twice.Vertices) == len(m.Vertices) and len(twice.Triangles) == 6 * nt
    t2 = twice.Topology()
    assert t2.Components == 1 and t2.NonManifoldEdges == t2.Edges and t2.IsWatertight
    assert len(K.Mesh.Concat([]).Vertices) == 0 and len(K.Mesh.Concat([]).Triangles) == 0
