"""Mesh topology on the MI355X (sdfk_trimesh_components / _topology / _select and their _device forms,
csrc/lib_trimesh_topology.hip) against the numpy model (tests/mesh_topology_model.py).  Every output is an integer (or a gathered
float) and unique given the input, so everything is compared for equality: labels, component rows, the census, the selection.
The meshes are small, tidy ones (tests/mesh_topology_cases.py): the hand-made shapes, sizes on both sides of a 256-lane block, of
the 2048-record sort tile and scan block, of the third key byte, deep label trees, 300 components.  No edge here has more than 3
triangles; random index soups, an edge of 5000 triangles (a run longer than a sort tile) and 70 000 components are in
tests/test_gpu_mesh_stress.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import MeshSdf
from tests import mesh_topology_cases as Cs
from tests import mesh_topology_model as M

pytestmark = pytest.mark.gpu
f32, i32, i64 = np.float32, np.int32, np.int64


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _check_selection(got, want, what):
    assert np.array_equal(got.VertexIndex, want.vertex_index) and got.VertexIndex.dtype == i32, what
    assert np.array_equal(got.TriangleIndex, want.triangle_index), what
    assert np.array_equal(got.Triangles, want.triangles) and got.Triangles.dtype == i32, what
    assert np.array_equal(_bits(got.Vertices), _bits(want.vertices)), what
    assert np.array_equal(_bits(got.Colors), _bits(want.colors)), what


def _check(V, T, colors=None, what="", keeps=()):
    """Components, Topology and Select of the host forms equal the model -> (handle, model topology, MeshComponents)."""
    t = MeshSdf((V, T, colors) if colors is not None else (V, T))
    want = M.topology(V, T)
    c = t.Components()
    assert c.Count == want.count, what
    assert c.VertexLabels.dtype == i32 and np.array_equal(c.VertexLabels, want.vertex), what
    assert c.TriangleLabels.dtype == i32 and np.array_equal(c.TriangleLabels, want.triangle), what
    assert c.Rows.dtype == i64 and np.array_equal(c.Rows, want.rows), (what, c.Rows[:4], want.rows[:4])
    for name, col in zip(("Triangles", "Vertices", "Edges", "BoundaryEdges", "NonManifoldEdges", "OddEdges", "InconsistentEdges", "AreaWeights"), range(8)):
        assert np.array_equal(getattr(c, name), want.rows[:, col]), (what, name)
    assert np.array_equal(c.EulerCharacteristic, [M.euler(r) for r in want.rows]), what
    assert np.array_equal(c.IsWatertight, [M.watertight(r) for r in want.rows]) and np.array_equal(c.IsOriented, [M.oriented(r) for r in want.rows]), what
    assert 1 <= c.Rounds <= len(V) + 1 and c.ShortcutLaunches >= 0, (what, c.Rounds)
    top = t.Topology()
    assert top.Census == want.census.tolist(), (what, top.Census, want.census)
    assert top.Triangles == len(T) - int(want.census[7]) and top.EulerCharacteristic == int(want.census[1] - want.census[2]) + top.Triangles
    assert top.IsWatertight == (want.census[5] == 0) and top.IsOriented == (want.census[6] == 0 and want.census[4] == 0)
    for keep in keeps:
        keep = np.resize(np.asarray(keep, bool), want.count)
        _check_selection(t.Select(keep), M.select(V, T, keep, colors=colors, topo=want), (what, keep[:8]))
    return t, want, c


# ---- the small shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.SMALL))
def test_small_shapes(gpu, name):
    V, T = Cs.SMALL[name]()
    _, want, c = _check(V, T, what=name, keeps=([True], [False], [True, False], [False, True]))
    if name in Cs.EXPECTED:
        assert c.Count == 1 and tuple(int(x) for x in c.Rows[0][:7]) == Cs.EXPECTED[name]
    if name == "two_tetrahedra_out_of_order":
        assert c.VertexLabels.tolist() == [0, 0, 0, 0, -1, 1, 1, 1, 1] and c.TriangleLabels.tolist() == [1] * 4 + [0] * 4
    if name == "with_degenerates":
        assert c.VertexLabels.tolist() == [0, 0, 0, -1, -1] and c.TriangleLabels.tolist() == [0, -1, -1]
        assert int(want.census[7]) == 2 and c.Rows[0][:7].tolist() == [1, 3, 3, 3, 0, 3, 0]
    if name == "no_area":
        assert c.Count == 2 and np.all(c.AreaWeights == 0)


def test_a_mesh_without_area_is_still_refused_by_the_sampler(gpu):
    """The topology calls make the sampling weights (all zero here) and keep them; sampling refuses the mesh as before, on either
    side of the topology call."""
    V, T = Cs.no_area()
    t = MeshSdf((V, T))
    with pytest.raises(N.SdfKitNativeError, match="no triangle has an area"):
        t.SamplePoints(5)
    assert np.all(t.Components().AreaWeights == 0)
    with pytest.raises(N.SdfKitNativeError, match="no triangle has an area"):
        t.SamplePoints(5)


# ---- sizes that straddle the machinery ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [255, 256, 257, 684, 685])
def test_block_tile_and_scan_edges(gpu, nv):
    """nv of 255 / 256 / 257: the last lane of a block, a full block, the first lane of the second.  nv of 684 / 685: nt of 682 / 683,
    where 3 nt crosses the 2048-record sort tile and the 2048-item scan block."""
    V, T = Cs.zigzag(nv)
    assert len(T) == nv - 2
    if nv >= 684:
        assert (3 * 682 <= 2048 < 3 * 683) and len(T) in (682, 683)
    _check(V, T, colors=Cs.vertex_colors(V), what=("zigzag", nv), keeps=([True], [False]))
    Vp, Tp = Cs.permuted(V, T, nv)
    _check(Vp, Tp, what=("zigzag permuted", nv), keeps=([True],))


def test_third_key_byte_and_many_rounds_grid(gpu):
    """A permuted 300 x 300 grid: nv = 90 000 > 65 536, so the third byte of each half of the edge key is live."""
    V, T = Cs.grid_permuted()
    assert len(V) > 65536
    _, want, c = _check(V, T, what="grid", keeps=([True],))
    assert c.Count == 1 and int(c.BoundaryEdges[0]) == 4 * 299


@functools.lru_cache(maxsize=None)
def _strip():
    return Cs.quad_strip(100000)


def test_long_strip_in_order(gpu):
    """The 100 000-quad strip, indices in order: the deep-tree case.  Observed on the MI355X: 2 hook rounds, 18 shortcut
    launches (the model's synchronous rounds: 2 and 17)."""
    V, T = _strip()
    _, want, c = _check(V, T, what="strip")
    print("strip in order: rounds", c.Rounds, "shortcut launches", c.ShortcutLaunches, "model", want.rounds, want.shortcuts)
    assert c.Count == 1 and c.Rounds <= len(V) + 1
    assert int(c.Edges[0]) == 400001 and int(c.BoundaryEdges[0]) == 200002


def test_long_strip_permuted(gpu):
    """The same strip with its indices permuted by a fixed seed: many rounds.  Observed on the MI355X: 12 hook rounds, 38
    shortcut launches (the model's synchronous rounds: 12 and 28)."""
    V, T = Cs.permuted(*_strip(), 7)
    _, want, c = _check(V, T, what="strip permuted", keeps=([True],))
    print("strip permuted: rounds", c.Rounds, "shortcut launches", c.ShortcutLaunches, "model", want.rounds, want.shortcuts)
    assert c.Count == 1 and c.Rounds <= len(V) + 1


def test_many_components_and_capacity(gpu):
    """300 disjoint tetrahedra, shuffled: a row per component, mixed waves, and capacity < C."""
    V, T = Cs.tetrahedra()
    rng = np.random.default_rng(5)
    t, want, c = _check(V, T, colors=Cs.vertex_colors(V), what="tetrahedra", keeps=([True], [False], [True, False, False], rng.random(300) < 0.5))
    assert c.Count == 300 and np.all(c.Rows[:, :7] == [4, 4, 6, 0, 0, 0, 0])
    for cap in (0, 1, 299, 300, 301):
        rows = np.full((302, 8), -7, i64)
        census = (C.c_int64 * 8)()
        N.check(N.lib().sdfk_trimesh_topology(t.handle, census, _vp(rows), cap))
        k = min(cap, 300)
        assert np.array_equal(rows[:k], want.rows[:k]) and np.all(rows[k:] == -7), cap
        assert census[:] == want.census.tolist(), cap
    # NULL outputs: each alone
    n = C.c_int64(-1)
    N.check(N.lib().sdfk_trimesh_components(t.handle, None, None, C.byref(n), None))
    assert n.value == 300
    N.check(N.lib().sdfk_trimesh_topology(t.handle, None, None, 300))
    vl = np.full(len(V) + 1, -7, i32)
    N.check(N.lib().sdfk_trimesh_components(t.handle, _vp(vl), None, None, None))
    assert np.array_equal(vl[:-1], want.vertex) and vl[-1] == -7


# ---- a real pipeline mesh -------------------------------------------------------------------------------------------------------
def test_pipeline_mesh_specks(gpu):
    """Two separated spheres and a tiny one, 48^3, through ToMesh: three closed oriented components; the cleaning calls equal the
    model's selection; the cleaned mesh goes back into a volume."""
    E = K.SdfExprs
    scene = E.Union(E.Union(E.Sphere(0.45, (1.0, 0.2, 0.2)).Translate(-0.6, 0.0, 0.0), E.Sphere(0.35, (0.2, 1.0, 0.2)).Translate(0.6, 0.1, 0.0)),
                    E.Sphere(0.12, (0.2, 0.2, 1.0)).Translate(0.0, 0.7, 0.5))
    m = scene.ToSdf().ToMesh([-1.2] * 3, [1.2] * 3, 48, 48, 48)
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, i32).reshape(-1, 3)
    want = M.topology(V, T)
    c = m.Components()
    assert c.Count == 3 == want.count and np.array_equal(c.Rows, want.rows)
    assert np.all(c.IsWatertight) and np.all(c.IsOriented) and np.all(c.EulerCharacteristic == 2)
    top = m.Topology()
    assert top.Census == want.census.tolist() and top.IsWatertight and top.IsOriented and top.EulerCharacteristic == 6
    small = int(c.Triangles.min())
    assert small < int(np.sort(c.Triangles)[1])
    for got, keep in ((m.LargestComponent(), np.arange(3) == M.largest(want.rows)),
                      (m.RemoveSmallComponents(minTriangles=small + 1), M.keep_small_removed(want.rows, small + 1)),
                      (m.RemoveSmallComponents(minAreaFraction=0.2), M.keep_small_removed(want.rows, 0, 0.2)),
                      (m.SelectComponents([False, True, True]), np.array([False, True, True]))):
        s = M.select(V, T, keep, colors=np.array(m.Colors, f32), topo=want)
        assert len(s.vertex_index) and np.array_equal(np.asarray(got.Triangles), s.triangles)
        assert np.array_equal(_bits(got.Vertices), _bits(s.vertices)) and np.array_equal(_bits(got.Colors), _bits(s.colors))
        assert np.array_equal(_bits(got.Normals), _bits(np.array(m.Normals, f32)[s.vertex_index]))
        assert np.array_equal(got.Min, s.vertices.min(axis=0)) and np.array_equal(got.Max, s.vertices.max(axis=0))
    assert int(np.count_nonzero(M.keep_small_removed(want.rows, small + 1))) == 2
    clean = m.RemoveSmallComponents(minTriangles=small + 1)
    assert clean.Topology().Components == 2
    vox = clean.ToVoxels([-1.2] * 3, [1.2] * 3, 24, 24, 24, maxDistance=0.3)
    vals = np.asarray(vox.Values)
    assert np.all(np.isfinite(vals)) and vals.min() < 0 < vals.max()
    empty = m.SelectComponents([False] * 3)
    assert len(empty.Vertices) == 0 and len(empty.Triangles) == 0 and empty.Vertices.shape == (0, 3)


# ---- select ---------------------------------------------------------------------------------------------------------------------
def test_select_none_all_and_untouched_tails(gpu):
    V, T = Cs.two_tetrahedra_out_of_order()
    T = np.concatenate([T, np.array([[4, 4, 0]], i32)])   # an index-degenerate triangle on the unreferenced vertex
    cols = Cs.vertex_colors(V)
    t, want, _ = _check(V, T, colors=cols, what="select")
    none = t.Select([False, False])
    assert len(none.VertexIndex) == len(none.TriangleIndex) == len(none.Triangles) == 0 and none.Vertices.shape == (0, 3)
    every = t.Select([True, True])
    assert every.VertexIndex.tolist() == [0, 1, 2, 3, 5, 6, 7, 8] and every.TriangleIndex.tolist() == list(range(8))   # (minus label -1)
    # raw: the entries beyond the counts stay as they were, and every output may be NULL
    nv, nt = len(V), len(T)
    bufs = {"vi": np.full(nv, -7, i32), "ti": np.full(nt, -7, i32), "tr": np.full(3 * nt, -7, i32), "vs": np.full((nv, 3), -7, f32), "cs": np.full((nv, 3), -7, f32)}
    keep = np.array([0, 1], np.uint8)
    kv, kt = C.c_int64(), C.c_int64()
    N.check(N.lib().sdfk_trimesh_select(t.handle, _vp(keep), *[_vp(b) for b in bufs.values()], C.byref(kv), C.byref(kt)))
    s = M.select(V, T, keep, colors=cols, topo=want)
    assert (kv.value, kt.value) == (4, 4)
    assert np.array_equal(bufs["vi"][:4], s.vertex_index) and np.all(bufs["vi"][4:] == -7)
    assert np.array_equal(bufs["ti"][:4], s.triangle_index) and np.all(bufs["ti"][4:] == -7)
    assert np.array_equal(bufs["tr"][:12], s.triangles) and np.all(bufs["tr"][12:] == -7)
    assert np.array_equal(_bits(bufs["vs"][:4]), _bits(s.vertices)) and np.all(bufs["vs"][4:] == -7)
    assert np.array_equal(_bits(bufs["cs"][:4]), _bits(s.colors)) and np.all(bufs["cs"][4:] == -7)
    N.check(N.lib().sdfk_trimesh_select(t.handle, _vp(keep), None, None, None, None, None, C.byref(kv), None))
    assert kv.value == 4


def test_device_forms_and_create_device_round_trip(gpu):
    """The _device forms give what the host forms give; the outputs of sdfk_trimesh_select_device go straight into
    sdfk_trimesh_create_device, and the topology of that handle is the model's for the selected mesh."""
    import torch
    N.bind_torch_stream()
    dev = torch.device("cuda", N._inited_device or 0)
    V, T = Cs.tetrahedra(40, seed=9)
    V2, T2 = Cs.permuted(*Cs.patch(9, 7), 2)
    V, T = np.concatenate([V, V2]), np.concatenate([T, T2 + len(V)]).astype(i32)
    cols = Cs.vertex_colors(V)
    t, want, _ = _check(V, T, colors=cols, what="device forms")
    nv, nt, Cn = len(V), len(T), want.count
    L = N.lib()
    vl, tl = torch.full((nv,), -7, dtype=torch.int32, device=dev), torch.full((nt,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((Cn + 1, 8), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    n, st, census = C.c_int64(), (C.c_int64 * 4)(), (C.c_int64 * 8)()
    N.check(L.sdfk_trimesh_components_device(t.handle, C.c_void_p(vl.data_ptr()), C.c_void_p(tl.data_ptr()), C.byref(n), st))
    N.check(L.sdfk_trimesh_topology_device(t.handle, census, C.c_void_p(rows.data_ptr()), Cn))
    N.check(L.sdfk_synchronize())
    assert n.value == Cn and st[0] >= 1 and st[2] == st[3] == 0
    assert np.array_equal(vl.cpu().numpy(), want.vertex) and np.array_equal(tl.cpu().numpy(), want.triangle)
    assert np.array_equal(rows.cpu().numpy()[:Cn], want.rows) and np.all(rows.cpu().numpy()[Cn] == -7) and census[:] == want.census.tolist()
    keep = (np.arange(Cn) % 3 != 1)
    kd = torch.from_numpy(keep.astype(np.uint8)).to(dev)
    vi, ti = torch.full((nv,), -7, dtype=torch.int32, device=dev), torch.full((nt,), -7, dtype=torch.int32, device=dev)
    tr = torch.full((3 * nt,), -7, dtype=torch.int32, device=dev)
    vs, cs = torch.full((nv, 3), -7.0, dtype=torch.float32, device=dev), torch.full((nv, 3), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    kv, kt = C.c_int64(), C.c_int64()
    N.check(L.sdfk_trimesh_select_device(t.handle, C.c_void_p(kd.data_ptr()), *[C.c_void_p(b.data_ptr()) for b in (vi, ti, tr, vs, cs)], C.byref(kv), C.byref(kt)))
    N.check(L.sdfk_synchronize())
    s = M.select(V, T, keep, colors=cols, topo=want)
    kv, kt = kv.value, kt.value
    assert (kv, kt) == (len(s.vertex_index), len(s.triangle_index)) and 0 < kv < nv
    assert np.array_equal(vi.cpu().numpy()[:kv], s.vertex_index) and np.all(vi.cpu().numpy()[kv:] == -7)
    assert np.array_equal(ti.cpu().numpy()[:kt], s.triangle_index) and np.array_equal(tr.cpu().numpy()[:3 * kt], s.triangles)
    assert np.all(tr.cpu().numpy()[3 * kt:] == -7)
    assert np.array_equal(_bits(vs.cpu().numpy()[:kv]), _bits(s.vertices)) and np.array_equal(_bits(cs.cpu().numpy()[:kv]), _bits(s.colors))
    h = C.c_void_p()
    N.check(L.sdfk_trimesh_create_device(C.c_void_p(vs.data_ptr()), kv, C.c_void_p(tr.data_ptr()), 3 * kt, C.c_void_p(cs.data_ptr()), C.byref(h)))
    try:
        want2 = M.topology(s.vertices, s.triangles)
        rows2 = np.zeros((want2.count, 8), i64)
        N.check(L.sdfk_trimesh_topology(h, census, _vp(rows2), want2.count))
        assert census[:] == want2.census.tolist() and np.array_equal(rows2, want2.rows)
        assert want2.count == int(np.count_nonzero(keep)) and np.array_equal(want2.rows, want.rows[keep])
    finally:
        L.sdfk_trimesh_free(h)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    V, T = Cs.tetrahedron()
    t = MeshSdf((V, T))
    L = N.lib()
    vl, tl = np.full(4, -7, i32), np.full(4, -7, i32)
    n, st = C.c_int64(-7), (C.c_int64 * 4)(-7, -7, -7, -7)
    census = (C.c_int64 * 8)(*([-7] * 8))
    rows = np.full((1, 8), -7, i64)
    bufs = [np.full(4, -7, i32), np.full(4, -7, i32), np.full(12, -7, i32), np.full((4, 3), -7, f32), np.full((4, 3), -7, f32)]
    kv, kt = C.c_int64(-7), C.c_int64(-7)
    keep = np.array([1], np.uint8)
    null = C.c_void_p()
    calls = {
        "components: null handle": lambda f: f(null, _vp(vl), _vp(tl), C.byref(n), st),
        "topology: null handle": lambda f: f(null, census, _vp(rows), 1),
        "topology: negative capacity": lambda f: f(t.handle, census, _vp(rows), -1),
        "select: null handle": lambda f: f(null, _vp(keep), *[_vp(b) for b in bufs], C.byref(kv), C.byref(kt)),
        "select: null keep": lambda f: f(t.handle, null, *[_vp(b) for b in bufs], C.byref(kv), C.byref(kt)),
    }
    for what, call in calls.items():
        name = "sdfk_trimesh_" + what.split(":")[0]
        for fn in (getattr(L, name), getattr(L, name + "_device")):   # (refused before any pointer is read: host arrays do for both)
            assert call(fn) == N.ERR_INVALID, what
            assert name in L.sdfk_last_error().decode(), what
    assert np.all(vl == -7) and np.all(tl == -7) and n.value == -7 and list(st) == [-7] * 4
    assert list(census) == [-7] * 8 and np.all(rows == -7) and all(np.all(b == -7) for b in bufs) and kv.value == kt.value == -7
    assert t.Components().Count == 1   # (the handle is as usable as before)
