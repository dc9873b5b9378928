"""Triangle-mesh distance volumes (MeshSdf, Mesh.ToVoxels; csrc/lib_trimesh.hip) on the MI355X against the numpy model
(tests/meshsdf_model.py): values, colours, triangle indices and closest points bit for bit, the sign against analytic SDFs on
closed meshes, the band, slabs, the device form, repeatability and refusals."""
import ctypes as C

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import MeshSdf
from tests import meshsdf_model as M
from tests import scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    bad = np.nonzero(a.view(np.uint32).reshape(-1) != b.view(np.uint32).reshape(-1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], a.reshape(-1)[bad[:5]], b.reshape(-1)[bad[:5]])


def _full(V, T, mn, mx, n, colors=None, band=np.inf):
    vox = MeshSdf((V, T, colors) if colors is not None else (V, T)).ToVoxels(mn, mx, *n, maxDistance=band)
    vals, cols = M.volume(V, T, mn, mx, n, colors=colors, band=band)
    _bits_equal(vox.Values, vals)
    if colors is not None:
        _bits_equal(vox.Colors, cols)
    return vox, vals


def _sampled(V, T, mn, mx, n, k, seed, colors=None, band=np.inf):
    vox = MeshSdf((V, T, colors) if colors is not None else (V, T)).ToVoxels(mn, mx, *n, maxDistance=band)
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.integers(0, n[a], k) for a in range(3)], 1)
    vals, cols = M.volume(V, T, mn, mx, n, colors=colors, band=band, sample=idx)
    got = vox.Values[idx[:, 0], idx[:, 1], idx[:, 2]]
    _bits_equal(got, vals)
    if colors is not None:
        _bits_equal(vox.Colors[idx[:, 0], idx[:, 1], idx[:, 2]], cols)
    return vox


def _centres(mn, mx, n):
    d, m = M.grid_constants(mn, mx, n)
    return [M.coord(m[a], np.arange(n[a]), d[a]) for a in range(3)]


def _mc_mesh(name, n, clip=True, lo=-2.5, hi=2.5):
    _, sdf = S.CATALOGUE[name]()
    m = sdf.ToMesh([lo] * 3, [hi] * 3, n, n, n, clipToBounds=clip)
    return np.array(m.Vertices, f32).reshape(-1, 3), np.array(m.Triangles, np.int32), np.array(m.Colors, f32).reshape(-1, 3)


def test_box_mesh_bitwise_and_against_analytic_box(gpu):
    V, T = M.box_mesh([-0.6, -0.45, -0.3], [0.6, 0.45, 0.3])
    mn, mx, n = [-1, -1, -1], [1, 1, 1], (20, 18, 16)
    vox, vals = _full(V, T, mn, mx, n)
    # Sdfs.Box (Sdf.cs:125-139) sampled on the same grid: equal within a few ulps of the half size, same sign off the surface
    box = K.Sdfs.Box(np.array([0.6, 0.45, 0.3], f32))
    ref = K.Voxels.SampleSdf(box, mn, mx, *n).Values
    assert np.max(np.abs(ref - vals)) <= 8 * np.spacing(f32(0.6))
    off = np.abs(ref) > 1e-5 * 2
    assert np.array_equal(np.sign(ref[off]), np.sign(vals[off]))


def test_octahedron_on_column_lattice(gpu):
    # vertices and edges exactly on cell-centre columns: first centre -0.9375, spacing 0.125 -> 0.0625 + k/8 ... use the
    # lattice of the centres themselves
    mn, mx, n = [-1, -1, -1], [1, 1, 1], (16, 16, 16)
    xs = _centres(mn, mx, n)[0]
    c = np.array([xs[8], xs[8], xs[8]], f32)
    r = f32(xs[13] - xs[8])
    V, T = M.octahedron(c, r)
    vox, vals = _full(V, T, mn, mx, n)
    # sign against the analytic octahedron |x|+|y|+|z| <= r, off the surface
    X, Y, Z = np.meshgrid(*_centres(mn, mx, n), indexing="ij")
    l1 = (np.abs(X - c[0]) + np.abs(Y - c[1]) + np.abs(Z - c[2])).astype(np.float64) - float(r)
    off = np.abs(vals) > 1e-5 * 2
    assert np.all((l1[off] < 0) == (vals[off] < 0))


def test_colored_scene_marching_cubes_mesh(gpu):
    V, T, Cc = _mc_mesh("colored_spheres", 48)
    assert np.any(Cc)
    _sampled(V, T, [-2.5] * 3, [2.5] * 3, (40, 36, 32), 1500, 1, colors=Cc)


def test_closed_marching_cubes_sphere_sign(gpu):
    V, T, _ = _mc_mesh("sphere_w", 40, lo=-1.5, hi=1.5)
    mn, mx, n = [-1.5] * 3, [1.5] * 3, (32, 32, 32)
    vox = MeshSdf((V, T)).ToVoxels(mn, mx, *n)
    vals = vox.Values
    X, Y, Z = np.meshgrid(*_centres(mn, mx, n), indexing="ij")
    ana = np.sqrt(X.astype(float) ** 2 + Y ** 2 + Z ** 2) - 1.0
    cell = 3.0 / 40
    ok = (np.abs(vals) > 1e-5 * 3) & (np.abs(ana) > cell)   # beyond the marching-cubes chord error
    assert np.all((ana[ok] < 0) == (vals[ok] < 0))
    assert np.count_nonzero(vals < 0) > 0


def test_closed_colored_scene_sign(gpu):
    """The clipped marching-cubes mesh of the coloured scene: off the surface, every voxel has the sign of the scene's SDF."""
    _, sdf = S.CATALOGUE["colored_spheres"]()
    lo, hi, n_mc = -2.5, 2.5, 48
    m = sdf.ToMesh([lo] * 3, [hi] * 3, n_mc, n_mc, n_mc, clipToBounds=True)
    V, T = np.array(m.Vertices, f32).reshape(-1, 3), np.array(m.Triangles, np.int32)
    cell = (hi - lo) / n_mc
    mn, mx, n = [lo + 2 * cell] * 3, [hi - 2 * cell] * 3, (36, 36, 36)   # (away from the clip faces)
    vals = MeshSdf((V, T)).ToVoxels(mn, mx, *n).Values
    ana = K.Voxels.SampleSdf(sdf, mn, mx, *n).Values
    ok = (np.abs(vals) > 1e-5 * (hi - lo)) & (np.abs(ana) > cell)
    assert np.all((ana[ok] < 0) == (vals[ok] < 0))
    assert np.count_nonzero(ok & (ana < 0)) > 30 and np.count_nonzero(ok & (ana > 0)) > 1000


def test_degenerate_and_duplicate_triangles(gpu):
    V, T = M.box_mesh([-0.5, -0.4, -0.3], [0.5, 0.4, 0.3])
    extra_v = np.array([[0.1, 0.1, 0.9], [0.1, 0.1, 0.9], [0.4, -0.2, 0.9], [0.7, 0.5, -0.9]], f32)
    Vd = np.concatenate([V, extra_v])
    Td = np.concatenate([T, T[:6], [8, 9, 10, 8, 8, 8, 8, 10, 11, 0, 0, 7]]).astype(np.int32)   # duplicates, zero area, a needle
    _full(Vd, Td, [-1] * 3, [1] * 3, (14, 12, 10))


def test_open_quad_is_deterministic_and_matches_model(gpu):
    V = np.array([[-0.5, -0.5, 0.1], [0.5, -0.5, 0.1], [0.5, 0.5, 0.2], [-0.5, 0.5, 0.2]], f32)
    T = np.array([0, 1, 2, 0, 2, 3], np.int32)
    vox, _ = _full(V, T, [-1] * 3, [1] * 3, (12, 12, 12))
    vox2 = MeshSdf((V, T)).ToVoxels([-1] * 3, [1] * 3, 12, 12, 12)
    _bits_equal(vox.Values, vox2.Values)


def test_slab_planes_equal_whole_volume(gpu):
    V, T, Cc = _mc_mesh("colored_spheres", 32)
    t = MeshSdf((V, T, Cc))
    mn, mx, n = [-2.5] * 3, [2.5] * 3, (24, 20, 28)
    whole = t.ToVoxels(mn, mx, *n)
    L = N.lib()
    h = C.c_void_p()
    z0, nzl = 9, 7
    N.check(L.sdfk_volume_create_slab(n[0], n[1], n[2], N.f3(mn), N.f3(mx), z0, nzl, 1, C.byref(h)))
    try:
        N.check(L.sdfk_trimesh_to_volume(t.handle, h, C.c_float(np.inf)))
        vals = np.empty((n[0], n[1], nzl), f32)
        cols = np.empty((n[0], n[1], nzl, 3), f32)
        N.check(L.sdfk_volume_download(h, C.c_void_p(vals.ctypes.data), C.c_void_p(cols.ctypes.data)))
    finally:
        L.sdfk_volume_free(h)
    _bits_equal(vals, whole.Values[:, :, z0:z0 + nzl])
    _bits_equal(cols, whole.Colors[:, :, z0:z0 + nzl])


def test_transformed_mesh(gpu):
    _, sdf = S.CATALOGUE["union8"]()
    m = sdf.ToMesh([-2.5] * 3, [2.5] * 3, 32, 32, 32, clipToBounds=True)
    M4 = np.eye(4, dtype=f32)
    M4[3, :3] = [0.25, -0.125, 0.5]
    m.Transform(M4)
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, np.int32)
    vox = m.ToVoxels([-2] * 3, [3] * 3, 24, 24, 24)
    rng = np.random.default_rng(5)
    idx = np.stack([rng.integers(0, 24, 800) for _ in range(3)], 1)
    vals, _ = M.volume(V, T, [-2] * 3, [3] * 3, (24, 24, 24), sample=idx)
    _bits_equal(vox.Values[idx[:, 0], idx[:, 1], idx[:, 2]], vals)


def test_band_clamps_and_keeps_in_band_values(gpu):
    V, T, Cc = _mc_mesh("colored_spheres", 40)
    t = MeshSdf((V, T, Cc))
    n = (32, 32, 32)
    full = t.ToVoxels([-2.5] * 3, [2.5] * 3, *n)
    band = f32(0.3)
    banded = t.ToVoxels([-2.5] * 3, [2.5] * 3, *n, maxDistance=band)
    a, b = full.Values, banded.Values
    inb = np.abs(a) <= band
    _bits_equal(b[inb], a[inb])
    _bits_equal(full.Colors[inb], banded.Colors[inb])
    assert np.all(np.abs(b[~inb]) == band) and np.array_equal(np.sign(b[~inb]), np.sign(a[~inb]))
    assert np.count_nonzero(~inb) > 0


def test_closest_queries_match_model(gpu):
    V, T, _ = _mc_mesh("union8", 40)
    rng = np.random.default_rng(9)
    Q = np.concatenate([rng.uniform(-3, 3, (600, 3)), V[rng.integers(0, len(V), 200)],
                        [[np.nan, 0, 0], [np.inf, 1, 1]]]).astype(f32)
    tri, dist, cp = MeshSdf((V, T)).Search(Q)
    rt, rd, rc, _, _ = M.closest(V, T, Q[:-2])
    assert np.array_equal(tri[:-2], rt)
    _bits_equal(dist[:-2], rd)
    _bits_equal(cp[:-2], rc)
    assert list(tri[-2:]) == [-1, -1] and np.all(np.isinf(dist[-2:]))


def test_device_form_equals_host_form(gpu):
    _, sdf = S.CATALOGUE["colored_spheres"]()
    L = N.lib()
    m = C.c_void_p()
    n = 40
    N.check(L.sdfk_sample_march(sdf.program(), N.f3([-2.5] * 3), N.f3([2.5] * 3), n, n, n, 1, C.c_float(0.0), 1, C.byref(m)))
    try:
        nv, ni = C.c_int64(), C.c_int64()
        N.check(L.sdfk_mesh_counts(m, C.byref(nv), C.byref(ni)))
        V = np.empty((nv.value, 3), f32)
        Cc = np.empty((nv.value, 3), f32)
        T = np.empty(ni.value, np.int32)
        N.check(L.sdfk_mesh_copy(m, C.c_void_p(V.ctypes.data), C.c_void_p(Cc.ctypes.data), None, C.c_void_p(T.ctypes.data)))
        vp, cp, tp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        N.check(L.sdfk_mesh_device_ptrs(m, C.byref(vp), C.byref(cp), None, C.byref(tp)))
        h = C.c_void_p()
        N.check(L.sdfk_trimesh_create_device(vp, nv.value, tp, ni.value, cp, C.byref(h)))
        dev = MeshSdf.__new__(MeshSdf)
        dev._h, dev.Colors = h, Cc
        a = dev.ToVoxels([-2.5] * 3, [2.5] * 3, 30, 30, 30)
    finally:
        L.sdfk_mesh_free(m)
    b = MeshSdf((V, T, Cc)).ToVoxels([-2.5] * 3, [2.5] * 3, 30, 30, 30)
    _bits_equal(a.Values, b.Values)
    _bits_equal(a.Colors, b.Colors)


def test_repeatable(gpu):
    V, T, Cc = _mc_mesh("union8", 40)
    t = MeshSdf((V, T, Cc))
    a = t.ToVoxels([-2.5] * 3, [2.5] * 3, 40, 40, 40)
    b = t.ToVoxels([-2.5] * 3, [2.5] * 3, 40, 40, 40)
    _bits_equal(a.Values, b.Values)
    _bits_equal(a.Colors, b.Colors)


def test_refusals(gpu):
    L = N.lib()
    V = np.zeros((3, 3), f32)
    V[1, 0] = V[2, 1] = 1

    def create(v, nv, t, ni):
        h = C.c_void_p()
        r = L.sdfk_trimesh_create(C.c_void_p(v.ctypes.data), nv, C.c_void_p(t.ctypes.data), ni, None, C.byref(h))
        if h.value:
            L.sdfk_trimesh_free(h)
        return r

    T = np.array([0, 1, 2], np.int32)
    assert create(V, 3, T, 3) == 0
    assert create(V, 3, T, 0) == N.ERR_INVALID
    assert create(V, 3, T, 2) == N.ERR_INVALID
    assert create(V, 3, np.array([0, 1, 3], np.int32), 3) == N.ERR_INVALID
    assert create(V, 3, np.array([0, -1, 2], np.int32), 3) == N.ERR_INVALID
    Vn = V.copy()
    Vn[2, 2] = np.nan
    assert create(Vn, 3, T, 3) == N.ERR_INVALID
    assert create(V, 3, T, 3 * (1 << 31)) == N.ERR_INVALID
    t = MeshSdf((V, T))
    vh = C.c_void_p()
    N.check(L.sdfk_volume_create(4, 4, 4, N.f3([-1] * 3), N.f3([1] * 3), 0, C.byref(vh)))
    try:
        assert L.sdfk_trimesh_to_volume(t.handle, vh, C.c_float(-1.0)) == N.ERR_INVALID
        assert L.sdfk_trimesh_to_volume(t.handle, vh, C.c_float(np.nan)) == N.ERR_INVALID
    finally:
        L.sdfk_volume_free(vh)


def test_large_sphere_mesh_into_256(gpu):
    _, sdf = S.CATALOGUE["sphere_w"]()
    m = sdf.ToMesh([-1.25] * 3, [1.25] * 3, 512, 512, 512, clipToBounds=True)
    V, T = np.array(m.Vertices, f32).reshape(-1, 3), np.array(m.Triangles, np.int32)
    assert len(T) // 3 > 800_000
    # a band of 8 voxels: the unbanded volume costs tens of seconds; in-band voxels are exact either way
    _sampled(V, T, [-1.25] * 3, [1.25] * 3, (256, 256, 256), 300, 13, band=f32(8 * 2.5 / 256))
