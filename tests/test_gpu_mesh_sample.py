"""Mesh.SamplePoints on the MI355X (sdfk_trimesh_sample[_device], csrc/lib_trimesh.hip: k_tm_area2, k_tm_sample_weights, the 64-bit
scan, k_tm_sample) against the numpy model (tests/mesh_sample_model.py), bit for bit, in both modes, on the smallest meshes at
which each part can go wrong (tests/mesh_sample_cases.py); meshes that are mostly degenerate -- random index soups, 300 of them
laid over each other -- are in tests/test_gpu_mesh_stress.py.  Nothing here has a tolerance of its own: points, normals, colours,
triangle indices, weights and stats are compared as bits; the two bounds that appear (2^-23 M for the distance of a sample from
its triangle; the registration residual) are the model's."""
import ctypes as C
import functools

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import MeshSdf
from tests import mesh_sample_cases as Cs
from tests import mesh_sample_model as S
from tests import meshsdf_model as MM

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FIELDS = ("Points", "Normals", "Colors", "Triangles", "Weights")


def _same(got, want, what=""):
    """Every output of a MeshSamples equal to the model's, as bits."""
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        if w is None:
            assert g is None, (what, name)
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        gb, wb = g.view(np.uint32).reshape(len(g), -1), w.view(np.uint32).reshape(len(w), -1)
        bad = np.flatnonzero(np.any(gb != wb, axis=1))
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def _check(V, T, n, seed=0, colors=None, handle=None, what=""):
    t = handle or MeshSdf((V, T, colors) if colors is not None else (V, T))
    for strat in (True, False):
        got = t.SamplePoints(n, seed, stratified=strat)
        _same(got, S.sample(V, T, n, seed, strat, colors=colors), (what, n, seed, strat))
    return t


@functools.lru_cache(maxsize=None)
def _sphere():
    """A marching-cubes sphere of 24^3 made on the device, with a colour per vertex that varies over it."""
    m = K.Sdfs.Sphere(1.0).ToMesh([-1.5] * 3, [1.5] * 3, 24, 24, 24)
    V, T, Nv = np.array(m.Vertices, f32), np.array(m.Triangles, np.int32), np.array(m.Normals, f32)
    assert len(T) // 3 > 2048
    return V, T, Nv, Cs.vertex_colors(V)


# ---- the cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257])
def test_one_triangle(gpu, n):
    """n = 257: the second block of k_tm_sample."""
    V, T = Cs.one_triangle()
    t = _check(V, T, n, seed=11)
    assert t.sample_stats() == {"sampled_triangles": 1, "total_weight": 1 << 32}


def test_weight_quantisation(gpu):
    """Copies of the unit triangle scaled by 2^-16 have weight exactly 1, those scaled by 2^-17 exactly 0 and never appear."""
    V, T = Cs.weight_quantisation()
    w, W = S.weights(V, T)
    assert w.tolist() == [0, 0, 1 << 32, 1, 0, 0, 1, 0]
    t = _check(V, T, 70001, seed=2)
    assert t.sample_stats() == {"sampled_triangles": 3, "total_weight": (1 << 32) + 2} and S.stats(V, T) == (3, (1 << 32) + 2)
    # (the two triangles of weight 1 own one unit in 2^32 each: they show in the stats; the weight-0 copies can never appear)
    for strat in (True, False):
        tri = t.SamplePoints(70001, 2, stratified=strat).Triangles
        assert set(tri.tolist()) <= {2, 3, 6} and not set(tri.tolist()) & {0, 1, 4, 5, 7}


def test_zero_area_triangles_interleaved(gpu):
    V, T = Cs.degenerate_interleaved()
    w, _ = S.weights(V, T)
    assert np.all(w[::2] == 0) and w[39] == 0 and np.all(w[1:39:2] > 0)
    t = _check(V, T, 30011, seed=3)
    tri = t.SamplePoints(30011, 3).Triangles
    assert set(tri.tolist()) == set(range(1, 39, 2))
    assert t.sample_stats()["sampled_triangles"] == 19


@pytest.mark.parametrize("n", [100003, 3])
def test_sheet_of_5000_triangles(gpu, n):
    """More than one block of the scan (2048 values each).  n = 3: fewer samples than triangles, the strata at their widest."""
    V, T = Cs.sheet()
    assert len(T) // 3 == 5000
    t = _check(V, T, n, seed=5, colors=Cs.vertex_colors(V))
    nz, total = S.stats(V, T)
    assert t.sample_stats() == {"sampled_triangles": nz, "total_weight": total} and nz == 5000


def test_marching_cubes_sphere_with_colours(gpu):
    """Colours and Weights bit-equal; blending the mesh's vertex normals in numpy with Triangles / Weights reproduces the formula
    of the colour blend, bit for bit, against the model's."""
    V, T, Nv, cols = _sphere()
    t = _check(V, T, 20011, seed=6, colors=cols)
    got = t.SamplePoints(20011, 6)
    ref = S.sample(V, T, 20011, 6, True, colors=cols)
    tri = T.reshape(-1, 3)[got.Triangles]
    wa, wb, wc = [got.Weights[:, k:k + 1] for k in range(3)]
    blended = (Nv[tri[:, 0]] * wa + Nv[tri[:, 1]] * wb) + Nv[tri[:, 2]] * wc
    want = MM.blend(Nv[tri[:, 0]], Nv[tri[:, 1]], Nv[tri[:, 2]], ref.w)
    assert np.array_equal(blended.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(((cols[tri[:, 0]] * wa + cols[tri[:, 1]] * wb) + cols[tri[:, 2]] * wc).view(np.uint32), got.Colors.view(np.uint32))
    assert np.all(np.sum(blended.astype(f64) * got.Normals, 1) > 0)          # the face normals point the way the vertex normals do


@pytest.mark.parametrize("case", ["far", "subnormal"])
def test_far_and_subnormal_coordinates(gpu, case):
    V, T, _, cols = _sphere()
    if case == "far":
        V = (V + np.array([4096.0, -8192.0, 1024.0], f32)).astype(f32)
    else:
        V = (V.astype(f64) * 2.0 ** -130).astype(f32)
        assert np.all(np.abs(V) < np.finfo(f32).tiny) and len(np.unique(V)) > 16
    _check(V, T, 5003, seed=7, colors=cols, what=case)


def test_seeds(gpu):
    V, T = Cs.sheet()
    t = MeshSdf((V, T))
    for seed in (0, 2 ** 64 - 1, 0x1234, 0x1234 ^ (1 << 40)):
        _check(V, T, 1001, seed=seed, handle=t)
    a, b = t.SamplePoints(1001, 0x1234), t.SamplePoints(1001, 0x1234 ^ (1 << 40))
    assert not np.array_equal(a.Points, b.Points) and not np.array_equal(a.Weights, b.Weights)
    a, b = t.SamplePoints(1001, 0, stratified=False), t.SamplePoints(1001, 2 ** 64 - 1, stratified=False)
    assert not np.array_equal(a.Triangles, b.Triangles)
    # plain mode: sample s does not depend on n
    assert np.array_equal(t.SamplePoints(1001, 9, stratified=False).Points[:300], t.SamplePoints(300, 9, stratified=False).Points)


def test_second_call_is_bit_equal(gpu):
    """The second call reads the W the first one cached on the handle."""
    V, T, _, cols = _sphere()
    t = MeshSdf((V, T, cols))
    a, b = t.SamplePoints(4001, 8), t.SamplePoints(4001, 8)
    _same(a, b)
    _same(a, S.sample(V, T, 4001, 8, True, colors=cols))


def test_device_form_equals_host_form_and_search_is_unchanged(gpu):
    import torch
    V, T, _, cols = _sphere()
    N.bind_torch_stream()
    t = MeshSdf((V, T, cols))
    Q = np.random.default_rng(1).uniform(-1.5, 1.5, (500, 3)).astype(f32)
    before = t.Search(Q)
    n = 3001
    dev = torch.device("cuda", N._inited_device or 0)
    for strat in (True, False):
        host = t.SamplePoints(n, 21, stratified=strat)
        bufs = [torch.zeros((n, 3), dtype=torch.float32, device=dev) for _ in range(3)] + [torch.zeros(n, dtype=torch.int32, device=dev),
                                                                                         torch.zeros((n, 3), dtype=torch.float32, device=dev)]
        torch.cuda.synchronize()
        t.SamplePointsDevice(n, 21, strat, *[b.data_ptr() for b in bufs])
        N.check(N.lib().sdfk_synchronize())
        _same(K.MeshSamples(*[b.cpu().numpy() for b in bufs]), host, ("device form", strat))
    after = t.Search(Q)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _raw(t, n, seed, flags, want):
    """sdfk_trimesh_sample with only the outputs named in `want`, each guarded by a sentinel row -> dict of arrays."""
    bufs = {"Points": np.full((n + 1, 3), -7, f32), "Normals": np.full((n + 1, 3), -7, f32), "Colors": np.full((n + 1, 3), -7, f32),
            "Triangles": np.full(n + 1, -7, np.int32), "Weights": np.full((n + 1, 3), -7, f32)}
    args = [C.c_void_p(bufs[k].ctypes.data) if k in want else C.c_void_p() for k in FIELDS]
    st = N.lib().sdfk_trimesh_sample(t.handle, n, C.c_uint64(seed), flags, *args, None)
    return st, bufs


def test_null_outputs_and_n_zero(gpu):
    V, T = Cs.sheet()
    cols = Cs.vertex_colors(V)
    t = MeshSdf((V, T, cols))
    n = 777
    ref = S.sample(V, T, n, 4, True, colors=cols)
    for only in FIELDS:
        st, bufs = _raw(t, n, 4, 1, {only})
        assert st == 0
        for k in FIELDS:
            if k == only:
                assert np.array_equal(bufs[k][:n].view(np.uint32), np.ascontiguousarray(getattr(ref, k)).view(np.uint32)), k
            else:
                assert np.all(bufs[k][:n] == -7), k
            assert np.all(bufs[k][n] == -7), k
    st, bufs = _raw(t, 0, 4, 1, set(FIELDS))
    assert st == 0 and all(np.all(b == -7) for b in bufs.values())
    got = t.SamplePoints(0)
    assert got.Points.shape == (0, 3) and got.Triangles.shape == (0,)
    # a mesh without colours: zeros
    st, bufs = _raw(MeshSdf((V, T)), n, 4, 1, {"Colors"})
    assert st == 0 and np.all(bufs["Colors"][:n] == 0) and not np.any(np.signbit(bufs["Colors"][:n]))


def test_refusals(gpu):
    V, T = Cs.one_triangle()
    t = MeshSdf((V, T))
    for n, flags in ((-1, 0), (2 ** 31, 0), (5, 2), (5, 3), (5, -1)):
        pts = np.full((8, 3), -7, f32)
        st = N.lib().sdfk_trimesh_sample(t.handle, n, C.c_uint64(0), flags, C.c_void_p(pts.ctypes.data), None, None, None, None, None)
        assert st == N.ERR_INVALID and np.all(pts == -7), (n, flags, st)
    for n in (-1, 2 ** 31):
        with pytest.raises(N.SdfKitNativeError) as e:
            t.SamplePoints(n)
        assert e.value.status == N.ERR_INVALID
    # a mesh in which no triangle has an area: refused with the stated message, the handle still answers Search
    V, T = Cs.all_degenerate()
    t = MeshSdf((V, T))
    for _ in range(2):
        with pytest.raises(N.SdfKitNativeError) as e:
            t.SamplePoints(10)
        assert e.value.status == N.ERR_INVALID and "no triangle has an area" in str(e.value)
    Q = np.array([[2, 2, 3], [0.5, 0, 1], [-1, 4, 0.25]], f32)
    tri, dist, cp = t.Search(Q)
    rt, rd, rc, _, _ = MM.closest(V, T, Q)
    assert np.array_equal(tri, rt) and np.array_equal(dist.view(np.uint32), rd.view(np.uint32)) and np.array_equal(cp.view(np.uint32), rc.view(np.uint32))


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _register(static, dynamic):
    """Point-to-plane registration of the moved dynamic samples onto the static samples -> (total, moved points, iterations)."""
    icp = K.IterativeClosestPoint(static.Points)
    icp.StaticNormals = static.Normals
    pts = dynamic.copy()
    total = icp.RegisterPoints(pts, metric="plane")
    return total, pts, icp.Iterations


def test_end_to_end_registration(gpu):
    """SamplePoints(4000) of the 24^3 sphere mesh with its normals as the static cloud; SamplePoints(1500, seed=1), moved by a
    small rigid transform, as the dynamic one; point-to-plane registration brings it back onto the surface.  How close is not
    set here: it is what the same registration reaches from the numpy model's samples -- equal, since the inputs are bit-equal --
    and that figure is recorded in tests/golden/mesh_sample_cases.json ("icp")."""
    from tests import icp_plane_model as IM
    V, T, _, _ = _sphere()
    t = MeshSdf((V, T))
    static, dyn = t.SamplePoints(4000), t.SamplePoints(1500, seed=1)
    m_static, m_dyn = S.sample(V, T, 4000, 0, True), S.sample(V, T, 1500, 1, True)
    _same(static, m_static)
    _same(dyn, m_dyn)
    # every sample lies on its triangle: within 2^-23 M of the mesh (M: the largest coordinate of the triangle)
    tri = T.reshape(-1, 3)[static.Triangles]
    M = np.max(np.abs(np.concatenate([V[tri[:, 0]], V[tri[:, 1]], V[tri[:, 2]]], 1)), 1).astype(f64)
    dist = t.Search(static.Points)[1].astype(f64)
    print("worst distance / (2^-23 M)", (dist / (2.0 ** -23 * M)).max())
    assert np.all(dist <= 2.0 ** -23 * M)
    R = IM._rodrigues(np.array([0.01, -0.02, 0.015]))
    moved = (dyn.Points.astype(f64) @ R.T + np.array([0.02, -0.015, 0.01])).astype(f32)
    before = float(np.sqrt(np.mean(t.Search(moved)[1].astype(f64) ** 2)))
    total, pts, iters = _register(static, moved)
    m_total, m_pts, m_iters = _register(m_static, moved)
    assert np.array_equal(total.view(np.uint32), m_total.view(np.uint32)) and np.array_equal(pts.view(np.uint32), m_pts.view(np.uint32))
    assert iters == m_iters
    residual = float(np.sqrt(np.mean(t.Search(pts)[1].astype(f64) ** 2)))
    m_residual = float(np.sqrt(np.mean(t.Search(m_pts)[1].astype(f64) ** 2)))
    print("rms distance to the mesh: before", before, "after", residual, "iterations", iters, "recorded:", {"residual": residual.hex(), "iterations": iters})
    rec = Cs.load()["icp"]
    assert residual == m_residual == float.fromhex(rec["residual"]) and iters == rec["iterations"]
    assert residual < before
