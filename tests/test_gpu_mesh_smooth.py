"""Mesh adjacency, smoothing and vertex normals on the MI355X (sdfk_trimesh_adjacency / _smooth / _vertex_normals and their
_device forms, csrc/lib_trimesh_smooth.hip) against the numpy model (tests/mesh_smooth_model.py).  Every output is one stated
function of the input, so everything is compared as bits or integers.  The meshes are small, tidy ones
(tests/mesh_smooth_cases.py): the hand-made shapes, a vertex whose degree crosses a block, sizes on both sides of the
2048-record sort tile for both sorts, of the third key byte, a permuted grid, a marching-cubes sphere far from the origin and at
subnormal scale.  On all of them any order of a vertex's adds rounds to the same float32, and no vertex has more than 301
neighbours; hubs of 5001 neighbours and 5000 corners (runs longer than a sort tile), random index soups and the mesh on which
only the stated order of the adds gives the right bits are in tests/test_gpu_mesh_stress.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import MeshSdf
from tests import mesh_smooth_cases as Cs
from tests import mesh_smooth_model as M

pytestmark = pytest.mark.gpu
f32, f64, i32, i64, u32, u8 = np.float32, np.float64, np.int32, np.int64, np.uint32, np.uint8

TAUBIN, LAPLACE = (0.5, -0.53), (0.5, 0.0)
ITERATIONS = (0, 1, 2, 7)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _check_adjacency(t, V, T, what):
    want = M.adjacency(len(V), T)
    got = t.Adjacency()
    assert got.Start.dtype == u32 and np.array_equal(got.Start, want.start), what
    assert got.Neighbors.dtype == u32 and np.array_equal(got.Neighbors, want.neighbors), what
    assert got.Boundary.dtype == u8 and np.array_equal(got.Boundary, want.boundary), what
    assert np.array_equal(got.Degree, want.degree), what
    return want


def _model_runs(V, T, lam, mu, pin, adj):
    """The model's positions after each of ITERATIONS, computed once along the way."""
    pinned = adj.boundary != 0 if pin else None
    P, out = np.ascontiguousarray(V, f32).copy(), {}
    for k in range(max(ITERATIONS) + 1):
        if k in ITERATIONS:
            out[k] = P
        P = M.step(P, adj, lam, pinned)
        if f32(mu) != 0:
            P = M.step(P, adj, mu, pinned)
    return out


def _check_smooth(t, V, T, adj, what, factors=(TAUBIN, LAPLACE), pins=(True, False)):
    cor = M.corners(len(V), T)
    for lam, mu in factors:
        for pin in pins:
            want = _model_runs(V, T, lam, mu, pin, adj)
            for k in ITERATIONS:
                got = t.Smooth(k, lam, mu, pin)
                assert got.dtype == f32 and np.array_equal(_bits(got), _bits(want[k])), (what, lam, mu, pin, k)
            # the normals of the smoothed positions cost no new handle
            assert np.array_equal(_bits(t.VertexNormals(want[7])), _bits(M.vertex_normals(want[7], T, cor=cor))), (what, lam, mu, pin)
    assert np.array_equal(_bits(t.VertexNormals()), _bits(M.vertex_normals(V, T, cor=cor))), what
    assert np.array_equal(_bits(t.VertexNormals(flip=True)), _bits(M.vertex_normals(V, T, flip=True, cor=cor))), what


# ---- adjacency --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.SMALL))
def test_small_shapes(gpu, name):
    V, T = Cs.SMALL[name]()
    t = MeshSdf((V, T))
    adj = _check_adjacency(t, V, T, name)
    if name == "patch_5x3":
        rim = np.ones((4, 6), bool)
        rim[1:-1, 1:-1] = False
        assert np.array_equal(adj.boundary.reshape(4, 6) != 0, rim)
    if name in ("torus_6x5", "tetrahedron", "doubled_triangle"):
        assert not np.any(adj.boundary)
    if name == "doubled_triangle":
        assert t.Adjacency().Neighbors.tolist() == [1, 2, 0, 2, 0, 1]
    if name == "big_fan_300":
        assert int(t.Adjacency().Degree[0]) == 301
    if name == "two_tetrahedra_out_of_order":
        assert int(t.Adjacency().Degree[4]) == 0                     # the unreferenced vertex
    if name == "with_degenerates":
        assert t.Adjacency().Degree.tolist() == [2, 2, 2, 0, 0]       # (2, 2, 3) and (4, 4, 4) connect nothing
    _check_smooth(t, V, T, adj, name)


@pytest.mark.parametrize("nv", [343, 344, 684, 685])
def test_sort_tile_edges(gpu, nv):
    """nt = 341 / 342: 6 nt = 2046 / 2052 round the 2048-record sort tile of the neighbour sort.  nt = 682 / 683: 3 nt round it for the
    corner sort (and 6 nt round two tiles)."""
    V, T = Cs.zigzag(nv)
    assert len(T) == nv - 2 and (6 * 341 <= 2048 < 6 * 342) and (3 * 682 <= 2048 < 3 * 683)
    for W, S, what in ((V, T, "zigzag"), Cs.permuted(V, T, nv) + ("zigzag permuted",)):
        t = MeshSdf((W, S))
        adj = _check_adjacency(t, W, S, (what, nv))
        _check_smooth(t, W, S, adj, (what, nv), factors=(TAUBIN,), pins=(True,))


@pytest.mark.parametrize("nv", [65535, 65536, 65537])
def test_third_key_byte(gpu, nv):
    """nv - 1 and nv on both sides of 2^16: the third byte of `to` and of `from` (which also holds nv, for the records of
    index-degenerate triangles) joins the sort."""
    V, T = Cs.zigzag(nv)
    T = np.concatenate([T[:1000], np.array([[7, 7, 9], [nv - 1, nv - 1, nv - 1]], i32), T[1000:]])   # two index-degenerate triangles
    t = MeshSdf((V, T))
    adj = _check_adjacency(t, V, T, ("zigzag", nv))
    assert int(adj.degree.max()) == 4
    want = M.smooth(V, T, 2, *TAUBIN, True, adj=adj)
    assert np.array_equal(_bits(t.Smooth(2, *TAUBIN, True)), _bits(want))
    assert np.array_equal(_bits(t.VertexNormals(want)), _bits(M.vertex_normals(want, T)))
    if nv == 65536:
        V, T = Cs.quad_strip(32767)
        assert len(V) == 65536
        _check_adjacency(MeshSdf((V, T)), V, T, "quad strip")


@functools.lru_cache(maxsize=None)
def _grid():
    V, T = Cs.grid_permuted()
    return V, T, M.adjacency(len(V), T)


@pytest.mark.parametrize("factors", [TAUBIN, LAPLACE])
def test_permuted_grid(gpu, factors):
    V, T, adj = _grid()
    assert len(V) > 65536
    t = MeshSdf((V, T))
    if factors == TAUBIN:
        _check_adjacency(t, V, T, "grid")
        assert int(adj.boundary.sum()) == 4 * 299
    _check_smooth(t, V, T, adj, "grid", factors=(factors,))


# ---- a real pipeline mesh -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere():
    E = K.SdfExprs
    return E.Sphere(0.8, (1.0, 0.4, 0.2)).ToSdf().ToMesh([-1.0] * 3, [1.0] * 3, 24, 24, 24)


@pytest.mark.parametrize("where", ["moved", "tiny"])
def test_marching_cubes_sphere_far_and_tiny(gpu, where):
    m = _sphere()
    V, T, cols = np.array(m.Vertices, f32), np.array(m.Triangles, i32).reshape(-1, 3), np.array(m.Colors, f32)
    assert len(V) > 500 and np.any(cols)
    V = V + Cs.MOVED if where == "moved" else V * Cs.TINY
    t = MeshSdf((V, T, cols))
    adj = _check_adjacency(t, V, T, where)
    assert not np.any(adj.boundary)
    _check_smooth(t, V, T, adj, where, pins=(True,))
    if where == "tiny":
        assert np.all(np.abs(t.Smooth(2)) < np.finfo(f32).tiny)
        n = t.VertexNormals().astype(f64)
        assert np.all(np.abs(np.sqrt((n ** 2).sum(axis=1)) - 1) < 1e-6)


def test_cached_calls_and_an_unchanged_handle(gpu):
    """The second call on the handle (which has its adjacency by then) equals the first; the handle's own positions, grid and
    packed triangles are as before: Search gives the same bits, and smoothing again starts from the same positions."""
    V, T = Cs.noisy_icosphere()
    t = MeshSdf((V, T))
    q = np.array([[0.1, 0.2, 0.3], [2.0, -1.0, 0.5], [0.0, 0.0, 0.0], [-0.7, 0.7, 0.1]], f32)
    before = t.Search(q)
    first = t.Smooth(7)
    adj1, n1 = t.Adjacency(), t.VertexNormals(first)
    second = t.Smooth(7)
    adj2, n2 = t.Adjacency(), t.VertexNormals(first)
    assert np.array_equal(_bits(first), _bits(second)) and np.array_equal(_bits(n1), _bits(n2))
    assert np.array_equal(adj1.Start, adj2.Start) and np.array_equal(adj1.Neighbors, adj2.Neighbors) and np.array_equal(adj1.Boundary, adj2.Boundary)
    after = t.Search(q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(_bits(before[1]), _bits(after[1])) and np.array_equal(_bits(before[2]), _bits(after[2]))
    assert np.array_equal(_bits(t.Smooth(0)), _bits(V))
    # a fresh handle agrees with the cached one, and smoothing does what it is for
    assert np.array_equal(_bits(MeshSdf((V, T)).Smooth(7)), _bits(first))
    assert Cs.radii(first)[0] < Cs.radii(V)[0]


def test_normals_without_area_flip_and_given_positions(gpu):
    V, T = Cs.no_area()
    t = MeshSdf((V, T))
    assert not np.any(_bits(t.VertexNormals())) and not np.any(_bits(t.VertexNormals(flip=True)))   # (+0, +0, +0)
    V, T = Cs.icosphere()
    t = MeshSdf((V, T))
    n = t.VertexNormals()
    assert np.array_equal(_bits(n), _bits(M.vertex_normals(V, T)))
    assert np.all((n.astype(f64) * V.astype(f64)).sum(axis=1) > 0)
    assert np.array_equal(_bits(t.VertexNormals(flip=True)), _bits(-n))
    # positions with an infinite coordinate: the vertices round it get zeros, nothing else changes
    W = V.copy()
    W[5, 1] = np.inf
    got, want = t.VertexNormals(W), M.vertex_normals(W, T)
    assert np.array_equal(_bits(got), _bits(want)) and not np.any(_bits(got[5])) and np.any(got != 0)
    with pytest.raises(ValueError):
        t.VertexNormals(V[:-1])


# ---- the _device forms ----------------------------------------------------------------------------------------------------------
def test_device_forms(gpu):
    import torch
    N.bind_torch_stream()
    dev = torch.device("cuda", N._inited_device or 0)
    V, T = Cs.noisy_icosphere()
    V2, T2 = Cs.permuted(*Cs.patch(9, 7), 2)
    V, T = np.concatenate([V, V2]), np.concatenate([T, T2 + len(V)]).astype(i32)
    nv = len(V)
    t = MeshSdf((V, T))
    want = M.adjacency(nv, T)
    L = N.lib()
    n = C.c_int64(-1)
    N.check(L.sdfk_trimesh_adjacency_device(t.handle, None, None, None, C.byref(n)))
    assert n.value == len(want.neighbors)
    start = torch.full((nv + 2,), 7, dtype=torch.int32, device=dev)
    nbr = torch.full((n.value + 1,), 7, dtype=torch.int32, device=dev)
    bnd = torch.full((nv + 1,), 7, dtype=torch.uint8, device=dev)
    out = torch.full((nv + 1, 3), -7.0, dtype=torch.float32, device=dev)
    nrm = torch.full((nv + 1, 3), -7.0, dtype=torch.float32, device=dev)
    nrm2 = torch.full((nv + 1, 3), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    N.check(L.sdfk_trimesh_adjacency_device(t.handle, C.c_void_p(start.data_ptr()), C.c_void_p(nbr.data_ptr()), C.c_void_p(bnd.data_ptr()), None))
    t.SmoothDevice(7, 0.5, -0.53, True, out.data_ptr())
    t.VertexNormalsDevice(out.data_ptr(), True, nrm.data_ptr())     # straight from the smoothed device array
    t.VertexNormalsDevice(None, False, nrm2.data_ptr())
    N.check(L.sdfk_synchronize())
    s, b, w = start.cpu().numpy().view(u32), nbr.cpu().numpy().view(u32), bnd.cpu().numpy()
    assert np.array_equal(s[:-1], want.start) and s[-1] == 7 and np.array_equal(b[:-1], want.neighbors) and b[-1] == 7
    assert np.array_equal(w[:-1], want.boundary) and w[-1] == 7
    P = M.smooth(V, T, 7, 0.5, -0.53, True, adj=want)
    o = out.cpu().numpy()
    assert np.array_equal(_bits(o[:-1]), _bits(P)) and np.all(o[-1] == -7)
    assert np.array_equal(_bits(nrm.cpu().numpy()[:-1]), _bits(M.vertex_normals(P, T, flip=True))) and np.all(nrm.cpu().numpy()[-1] == -7)
    assert np.array_equal(_bits(nrm2.cpu().numpy()[:-1]), _bits(M.vertex_normals(V, T)))
    for k, (lam, mu) in ((0, TAUBIN), (1, LAPLACE), (1, TAUBIN), (2, LAPLACE)):   # 0, 1, 2, 2 steps: each parity of the ping-pong
        out.fill_(-7.0)
        torch.cuda.synchronize()
        t.SmoothDevice(k, lam, mu, False, out.data_ptr())
        N.check(L.sdfk_synchronize())
        assert np.array_equal(_bits(out.cpu().numpy()[:-1]), _bits(M.smooth(V, T, k, lam, mu, False, adj=want))), (k, lam, mu)
    # the smoothed device array goes straight into a new handle
    h = C.c_void_p()
    tri = torch.from_numpy(T.reshape(-1)).to(dev)
    t.SmoothDevice(7, 0.5, -0.53, True, out.data_ptr())
    N.check(L.sdfk_trimesh_create_device(C.c_void_p(out.data_ptr()), nv, C.c_void_p(tri.data_ptr()), tri.numel(), None, C.byref(h)))
    try:
        back = np.empty((nv, 3), f32)
        N.check(L.sdfk_trimesh_smooth(h, 0, 0.5, 0.0, 0, _vp(back)))
        assert np.array_equal(_bits(back), _bits(P))
    finally:
        L.sdfk_trimesh_free(h)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    V, T = Cs.tetrahedron()
    t = MeshSdf((V, T))
    L = N.lib()
    out = np.full((4, 3), -7, f32)
    start, nbr, bnd = np.full(5, 7, u32), np.full(12, 7, u32), np.full(4, 7, u8)
    n = C.c_int64(-7)
    null = C.c_void_p()
    fl = C.c_float
    calls = [
        ("adjacency", "null argument", lambda f: f(null, _vp(start), _vp(nbr), _vp(bnd), C.byref(n))),
        ("smooth", "null argument", lambda f: f(null, 1, fl(0.5), fl(0.0), 0, _vp(out))),
        ("smooth", "null output", lambda f: f(t.handle, 1, fl(0.5), fl(0.0), 0, null)),
        ("smooth", "iterations must be in", lambda f: f(t.handle, -1, fl(0.5), fl(0.0), 0, _vp(out))),
        ("smooth", "iterations must be in", lambda f: f(t.handle, 65537, fl(0.5), fl(0.0), 0, _vp(out))),
        ("smooth", "lambda and mu must be finite", lambda f: f(t.handle, 1, fl(np.nan), fl(0.0), 0, _vp(out))),
        ("smooth", "lambda and mu must be finite", lambda f: f(t.handle, 1, fl(0.5), fl(np.inf), 0, _vp(out))),
        ("smooth", "unknown flag bits", lambda f: f(t.handle, 1, fl(0.5), fl(0.0), 2, _vp(out))),
        ("vertex_normals", "null argument", lambda f: f(null, null, 0, _vp(out))),
        ("vertex_normals", "null output", lambda f: f(t.handle, null, 0, null)),
        ("vertex_normals", "unknown flag bits", lambda f: f(t.handle, null, 4, _vp(out))),
    ]
    for which, message, call in calls:
        name = "sdfk_trimesh_" + which
        for fn in (getattr(L, name), getattr(L, name + "_device")):   # (refused before any pointer is read: host arrays do for both)
            assert call(fn) == N.ERR_INVALID, (which, message)
            err = L.sdfk_last_error().decode()
            assert name in err and message in err, (which, message, err)
    assert np.all(out == -7) and np.all(start == 7) and np.all(nbr == 7) and np.all(bnd == 7) and n.value == -7
    assert np.array_equal(_bits(t.Smooth(1, 0.5, 0.0)), _bits(M.smooth(V, T, 1, 0.5, 0.0)))   # (the handle is as usable as before)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_mesh_smooth_and_recompute_normals_end_to_end(gpu):
    m = _sphere()
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, i32).reshape(-1, 3)
    old_normals = np.array(m.Normals, f32)
    s = m.Smooth()
    want = M.smooth(V, T, 10, 0.5, -0.53, True)
    assert s is not m and np.array_equal(np.asarray(s.Triangles), np.asarray(m.Triangles)) and np.array_equal(_bits(s.Colors), _bits(m.Colors))
    assert np.array_equal(_bits(s.Vertices), _bits(want)) and not np.array_equal(_bits(want), _bits(V))
    assert np.array_equal(_bits(s.Normals), _bits(M.vertex_normals(want, T)))
    assert np.array_equal(s.Min, want.min(axis=0)) and np.array_equal(s.Max, want.max(axis=0))
    assert np.array_equal(_bits(m.Vertices), _bits(V)) and np.array_equal(_bits(m.Normals), _bits(old_normals))   # the source mesh is untouched
    kept = m.Smooth(3, 0.5, 0.0, normals=False)
    assert np.array_equal(_bits(kept.Normals), _bits(old_normals)) and np.array_equal(_bits(kept.Vertices), _bits(M.smooth(V, T, 3, 0.5, 0.0, True)))
    # marching-cubes meshes wind with their gradient normals: nothing is flipped
    r = m.RecomputeNormals()
    unflipped = M.vertex_normals(V, T)
    assert M.side_votes(unflipped, old_normals) == (len(V), 0)
    assert np.array_equal(_bits(r.Normals), _bits(unflipped)) and np.array_equal(_bits(r.Vertices), _bits(V))
    assert np.array_equal(r.Min, m.Min) and np.array_equal(r.Max, m.Max) and np.array_equal(np.asarray(r.Triangles), np.asarray(m.Triangles))
    assert np.array_equal(_bits(m.RecomputeNormals(flip=True).Normals), _bits(M.vertex_normals(V, T, flip=True)))
    # present normals on the other side: kept there; a tie and unusable normals do not flip
    inward = K.Mesh(m.Vertices, m.Colors, -old_normals, m.Triangles, m.Min, m.Max)
    assert np.array_equal(_bits(inward.RecomputeNormals().Normals), _bits(M.vertex_normals(V, T, flip=True)))
    none = K.Mesh(m.Vertices, m.Colors, np.zeros_like(old_normals), m.Triangles, m.Min, m.Max)
    assert np.array_equal(_bits(none.RecomputeNormals().Normals), _bits(unflipped))
