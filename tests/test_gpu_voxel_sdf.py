"""Voxel volumes inside GPU SDF programs (SDFK_OP_VOXEL_NEAREST / SDFK_OP_VOXEL_LINEAR, sdfk_program_create_bound; Voxels[p],
Voxels.Sample / SampleColor / ToSdf) on the MI355X, bit for bit against the numpy model (tests/voxel_sdf_model.py): the sampler with
and without ClipToBounds, SdfEx.Sample, the ray marcher, meshes (stored = the oracle's marching of the model volume, elided and
culled = stored), random programs that mix volume reads into the IR, structure sharing, snapshot semantics, slabs and the node's
refusal."""
import ctypes as C

import numpy as np
import pytest

from oracle import ir_interp as I
from oracle import oracle as O
from sdfkit_amd import _native as N
from sdfkit_amd import MeshSdf, Sdfs, Voxels
from sdfkit_amd.api import Mesh, Sdf, _box_distance
from sdfkit_amd.expr import MathF, Vec4, trace_bound
from tests import voxel_sdf_model as M
from tests.test_gpu_parity import assert_mesh_equal

pytestmark = pytest.mark.gpu
f32 = np.float32


def _volume(rng, shape, mn, mx, colors=True, specials=True):
    vals = rng.uniform(-1, 1, shape).astype(f32)
    if specials and vals.size > 20:
        flat = vals.reshape(-1)
        flat[rng.integers(0, flat.size, 3)] = np.nan
        flat[rng.integers(0, flat.size, 2)] = np.inf
        flat[rng.integers(0, flat.size, 2)] = -np.inf
    cols = rng.uniform(0, 1, shape + (3,)).astype(f32) if colors else None
    return Voxels(vals, cols, mn, mx), (vals, cols, mn, mx)


def _model_vol(vox):
    cols = vox.Colors if vox._colors_present() else None
    return (vox.Values.copy(), None if cols is None else cols.copy(), vox.Min, vox.Max)


def _ops(sdf):
    ops, out, vols = trace_bound(sdf.fn, sdf.writes_color)
    return ops, out, vols


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _two_volume_sdf(v0, v1):
    """w = v0[p] + 0.5 v1.Sample(p), colour = (v1.SampleColor(p).x, .y, v0 nearest green)"""
    def fn(p):
        c = v1.SampleColor(p)
        g = p.x.b.voxel(M.NEAREST, v0, p, 1)
        return Vec4(c.x, c.y, g, v0[p] + v1.Sample(p) * 0.5)
    return Sdf(fn, True)


@pytest.fixture(scope="module")
def vols(gpu):
    rng = np.random.default_rng(11)
    v0, m0 = _volume(rng, (9, 1, 13), (-1.0, -0.25, -1.5), (1.25, 0.5, 1.0))     # an N = 1 axis
    v1, m1 = _volume(rng, (12, 10, 14), (-1.5, -1.0, -1.25), (1.0, 1.5, 1.25))
    return (v0, m0), (v1, m1)


@pytest.mark.parametrize("clip", [False, True])
def test_sampler_matches_model(vols, clip):
    (v0, m0), (v1, m1) = vols
    sdf = _two_volume_sdf(v0, v1)
    ops, out, bound = _ops(sdf)
    assert bound == [v1, v0] or bound == [v0, v1]
    mvols = [m0 if b is v0 else m1 for b in bound]
    mn, mx, n = (-2.0, -1.5, -2.0), (2.0, 1.75, 1.5), (37, 29, 33)   # the grid reaches past both volumes' boxes
    got = sdf.ToVoxels(mn, mx, *n, clipToBounds=clip)
    want_v, want_c = M.sample(ops, out, True, mn, mx, *n, mvols, clip=clip)
    assert _eq(got.Values, want_v)
    assert _eq(got.Colors, want_c)


def test_eval_points_matches_model(vols):
    (v0, m0), (v1, m1) = vols
    sdf = _two_volume_sdf(v0, v1)
    ops, out, bound = _ops(sdf)
    mvols = [m0 if b is v0 else m1 for b in bound]
    rng = np.random.default_rng(2)
    pts = [rng.uniform(-3, 3, (4000, 3))]
    for vol in (m0, m1):   # cell boundaries, centres, the box's faces
        d, mn = M.vol_d(vol), np.asarray(vol[2], f32)
        k = np.stack([rng.integers(-1, s + 2, 500) for s in vol[0].shape], -1)
        pts += [mn + k * d, mn + (k + f32(0.5)) * d, np.asarray(vol[3], f32)[None] + np.zeros((3, 3), f32)]
    pts = np.concatenate(pts).astype(f32)
    pts[:7, 0] = np.nan
    pts[7:14, 2] = np.nan
    pts[14:20] = [[np.inf, 0, 0], [-np.inf, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, -1e30, 1e30], [3e38, 3e38, -3e38]]
    got = sdf.Sample(pts)
    want = M.run(ops, out, pts, mvols)
    for k in range(4):
        assert _eq(got[:, k], want[k]), k


def test_raymarch_matches_model(gpu):
    # a smooth field: the distance of a sphere, sampled into a volume, plus its colours
    rng = np.random.default_rng(4)
    n = 24
    mn, mx = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)
    px, py, pz = M.grid_points(mn, mx, n, n, n)
    vals = (np.sqrt(px * px + py * py + pz * pz) - f32(1)).astype(f32)
    cols = rng.uniform(0, 1, (n, n, n, 3)).astype(f32)
    vox = Voxels(vals, cols, mn, mx)
    for interpolate in (True, False):
        sdf = vox.ToSdf(interpolate)
        ops, out, _ = _ops(sdf)
        w, h = 48, 32
        cam, vpi = O.ray_camera(O.look_at((0, 0, 5), (0, 0, 0), (0, 1, 0)), 60.0, w, h, 1.0, 100.0)
        depth, rgb = np.empty((h, w), f32), np.empty((h, w, 3), f32)
        N.check(N.lib().sdfk_raymarch(sdf.program(), w, h, N.f3(np.asarray(cam, f32).reshape(-1)),
                                      (C.c_float * 16)(*np.asarray(vpi, f32).reshape(-1)), C.c_float(1.0), C.c_float(100.0), 40,
                                      depth.ctypes.data, rgb.ctypes.data))
        md, mrgb = M.raymarch(ops, out, True, [(vals, cols, mn, mx)], w, h, cam, vpi, 1.0, 100.0, 40)
        assert _eq(depth, md)
        assert _eq(rgb, mrgb)
        assert np.sum(depth < 10) > 50   # (the sphere is in the picture)


@pytest.fixture(scope="module")
def mesh_vox(gpu):
    """the sphere mesh of the oracle turned into a banded distance volume (Mesh.ToVoxels)"""
    s = O.Scene(); s.sphere_w(1.0)
    ov, oc = O.sample(s, [-1.5] * 3, [1.5] * 3, 48, 48, 48)
    om = O.march(ov, oc, [-1.5] * 3, [1.5] * 3)
    ms = MeshSdf((om.vertices, om.triangles))
    return ms.ToVoxels([-1.25] * 3, [1.25] * 3, 40, 36, 44, maxDistance=0.25)


def test_solid_of_the_indexer_on_a_mesh_volume(mesh_vox):
    sdf = Sdfs.Solid(lambda p: mesh_vox[p])
    ops, out, _ = _ops(sdf)
    mvol = _model_vol(mesh_vox)
    mn, mx, n = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), (33, 35, 31)
    got = sdf.ToVoxels(mn, mx, *n, clipToBounds=False)
    want_v, want_c = M.sample(ops, out, True, mn, mx, *n, [mvol])
    assert _eq(got.Values, want_v) and _eq(got.Colors, want_c)
    assert np.all(got.Colors == 1.0)


def _union_with_box(vox, interpolate):
    def fn(p):
        a = vox.Sample(p) if interpolate else vox[p]
        return Vec4.of((1.0, 1.0, 1.0), MathF.Min(a, _box_distance(p.__class__(p.x - 0.75, p.y, p.z), (0.4, 0.3, 0.5))))
    return Sdf(fn, True)


@pytest.mark.parametrize("interpolate", [False, True])
def test_union_mesh_stored_is_the_oracles_and_elided_is_stored(mesh_vox, interpolate):
    sdf = _union_with_box(mesh_vox, interpolate)
    ops, out, _ = _ops(sdf)
    mvol = _model_vol(mesh_vox)
    mn, mx, dims = [-1.5] * 3, [1.5] * 3, (264, 260, 256)   # above the captured-graph limit: the elided path applies
    mv, mc = M.sample(ops, out, True, mn, mx, *dims, [mvol], clip=True)
    om = O.march(mv, mc, mn, mx)
    assert len(om.vertices) > 1000
    with N.option(N.OPT_ELIDE_VOLUME, 0):
        stored = sdf.ToMesh(mn, mx, *dims)
    assert_mesh_equal(stored, om)
    for mode in (2, 1):
        with N.option(N.OPT_ELIDE_VOLUME, mode):
            for _ in range(2):
                m = sdf.ToMesh(mn, mx, *dims)
                assert np.array_equal(m.Triangles, stored.Triangles)
                assert _eq(m.Vertices, stored.Vertices) and _eq(m.Colors, stored.Colors)


def _random_volume_program(seed, nvol):
    """ir_interp.random_program with volume reads mixed in: at the sample point, at random earlier values, and combined"""
    rng = np.random.default_rng(1000 + seed)
    ops, out = I.random_program(seed, n_ops=36)
    ops = list(ops)
    for _ in range(6):
        k = len(ops)
        slot, ch = int(rng.integers(0, nvol)), int(rng.choice([3, 3, 0, 2]))
        op = int(rng.choice([M.NEAREST, M.LINEAR]))
        if rng.random() < 0.6:
            a, b, c = 0, 1, 2
        else:
            a, b, c = (int(rng.integers(0, k)) for _ in range(3))
        ops.append((op, a, b, c, (slot << 2) | ch, 0.0))
        j = int(rng.integers(max(0, k - 8), k))
        ops.append((int(rng.choice([I.MIN_IEEE, I.ADD, I.MAX_SEL, I.MUL])), k, j, -1, -1, 0.0))
    n = len(ops)
    w = n - 1 if seed % 2 == 0 else n - 3
    return ops, [n - 2, out[1], n - 4, w]


@pytest.mark.parametrize("seed", range(6))
def test_random_volume_programs_elided_equals_stored(gpu, seed):
    rng = np.random.default_rng(seed)
    v0, m0 = _volume(rng, (20, 17, 23), (-2.0, -1.5, -1.75), (1.5, 2.0, 1.25), specials=seed % 3 == 0)
    v1, m1 = _volume(rng, (5, 9, 1), (-1.0, -1.0, -0.5), (1.0, 1.0, 0.5))
    vlist = [v0, v1]
    ops, out = _random_volume_program(seed, 2)
    arr = (N.Op * len(ops))()
    for i, (op, a, b, c, d, imm) in enumerate(ops):
        arr[i].opcode, arr[i].a, arr[i].b, arr[i].c, arr[i].d, arr[i].imm = op, a, b, c, d, imm
    hs = (C.c_void_p * 2)(*[v._sync_to_device().value for v in vlist])
    prog = C.c_void_p()
    N.check(N.lib().sdfk_program_create_bound(arr, len(ops), (C.c_int32 * 4)(*out), 1, hs, 2, C.byref(prog)))
    try:
        mn, mx, dims = (-2.5, -2.0, -2.25), (2.25, 2.5, 2.0), (272, 264, 256)
        meshes = {}
        for mode in (0, 2, 1):
            with N.option(N.OPT_ELIDE_VOLUME, mode):
                for clip in (1, 0):
                    h = C.c_void_p()
                    N.check(N.lib().sdfk_sample_march(prog, N.f3(mn), N.f3(mx), *dims, clip, C.c_float(0.0), 1, C.byref(h)))
                    meshes[(mode, clip)] = Mesh._from_handle(h)
        for clip in (1, 0):
            s = meshes[(0, clip)]
            for mode in (2, 1):
                m = meshes[(mode, clip)]
                assert np.array_equal(m.Triangles, s.Triangles), (mode, clip)
                assert _eq(m.Vertices, s.Vertices) and _eq(m.Colors, s.Colors), (mode, clip)
        # and the stored volume is the model's (a small grid: the whole program through sdfk_sample)
        vol = C.c_void_p()
        small = (23, 19, 21)
        N.check(N.lib().sdfk_volume_create(*small, N.f3(mn), N.f3(mx), 1, C.byref(vol)))
        try:
            N.check(N.lib().sdfk_sample(prog, vol, 0))
            gv, gc = np.empty(small, f32), np.empty(small + (3,), f32)
            N.check(N.lib().sdfk_volume_download(vol, gv.ctypes.data, gc.ctypes.data))
        finally:
            N.lib().sdfk_volume_free(vol)
        wv, wc = M.sample(ops, out, True, mn, mx, *small, [m0, m1])
        assert _eq(gv, wv) and _eq(gc, wc)
    finally:
        N.lib().sdfk_program_destroy(prog)


def test_another_volume_of_the_same_structure_compiles_nothing(gpu):
    rng = np.random.default_rng(8)
    a, _ = _volume(rng, (10, 11, 12), (-1, -1, -1), (1, 1, 1))
    b, mb = _volume(rng, (7, 13, 5), (-2, -1, 0), (0.5, 1.5, 2.5))
    pts = rng.uniform(-2, 2, (1000, 3)).astype(f32)
    a.ToSdf().Sample(pts)
    c0 = C.c_int64()
    N.check(N.lib().sdfk_jit_stats(C.byref(c0), None, None))
    sdf = b.ToSdf()
    got = sdf.Sample(pts)
    c1 = C.c_int64()
    N.check(N.lib().sdfk_jit_stats(C.byref(c1), None, None))
    assert c1.value == c0.value
    ops, out, _ = _ops(sdf)
    want = M.run(ops, out, pts, [mb])
    assert all(_eq(got[:, k], want[k]) for k in range(4))


def test_snapshot_and_version_counter(gpu):
    rng = np.random.default_rng(9)
    vals = rng.uniform(-1, 1, (8, 9, 10)).astype(f32)
    mn, mx = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    pts = rng.uniform(-1.2, 1.2, (500, 3)).astype(f32)
    # C ABI: the program keeps its copy whatever happens to the source volume
    vol = C.c_void_p()
    N.check(N.lib().sdfk_volume_create(8, 9, 10, N.f3(mn), N.f3(mx), 0, C.byref(vol)))
    N.check(N.lib().sdfk_volume_upload(vol, vals.ctypes.data, None))
    ops = [(1, -1, -1, -1, -1, 0.0), (2, -1, -1, -1, -1, 0.0), (3, -1, -1, -1, -1, 0.0), (M.LINEAR, 0, 1, 2, 3, 0.0)]
    arr = (N.Op * 4)()
    for i, (op, a, b, c, d, imm) in enumerate(ops):
        arr[i].opcode, arr[i].a, arr[i].b, arr[i].c, arr[i].d, arr[i].imm = op, a, b, c, d, imm
    prog = C.c_void_p()
    hs = (C.c_void_p * 1)(vol.value)
    N.check(N.lib().sdfk_program_create_bound(arr, 4, (C.c_int32 * 4)(-1, -1, -1, 3), 0, hs, 1, C.byref(prog)))
    want = M.run(ops, [-1, -1, -1, 3], pts, [(vals, None, mn, mx)])[3]
    out = np.zeros((len(pts), 4), f32)

    def points():
        N.check(N.lib().sdfk_eval_points(prog, pts.ctypes.data, len(pts), out.ctypes.data))
        return out[:, 3].copy()
    assert _eq(points(), want)
    N.check(N.lib().sdfk_volume_upload(vol, (vals * 2).astype(f32).ctypes.data, None))
    assert _eq(points(), want)
    N.check(N.lib().sdfk_sample(prog, vol, 0))       # sampled into the very volume it was built from
    got = np.empty((8, 9, 10), f32)
    N.check(N.lib().sdfk_volume_download(vol, got.ctypes.data, None))
    px, py, pz = M.grid_points(mn, mx, 8, 9, 10)
    assert _eq(got, M.linear((vals, None, mn, mx), 3, px, py, pz))
    N.lib().sdfk_volume_free(vol)
    assert _eq(points(), want)
    N.lib().sdfk_program_destroy(prog)
    # Python: an edit of the Voxels reaches the Sdf through the version counter
    vox = Voxels(vals.copy(), None, mn, mx)
    sdf = Sdfs.Solid(lambda p: vox.Sample(p))
    first = sdf.Sample(pts)[:, 3].copy()
    assert _eq(first, want)
    vox.Values[:] = -vals
    assert _eq(sdf.Sample(pts)[:, 3], M.linear((-vals, None, mn, mx), 3, pts[:, 0], pts[:, 1], pts[:, 2]))
    vox.SampleSdf(Sdfs.Sphere(0.5))
    sph = vox.Values.copy()
    assert _eq(sdf.Sample(pts)[:, 3], M.linear((sph, None, mn, mx), 3, pts[:, 0], pts[:, 1], pts[:, 2]))


def test_four_slabs_equal_the_whole_grid(mesh_vox):
    from tests.slab_worker import GpuSlabWorker
    sdf = _union_with_box(mesh_vox, True)
    mn, mx, n = [-1.5] * 3, [1.5] * 3, 96
    with N.option(N.OPT_ELIDE_VOLUME, 0):
        whole = sdf.ToMesh(mn, mx, n, n, n)
    verts, tris, base = [], [], 0
    for r in range(4):
        w = GpuSlabWorker(sdf, mn, mx, n, n, n, r, 4)
        try:
            nv, _ = w.run_local()
            m = Mesh._from_handle(w.mesh)
            w.mesh = None
            verts.append(m.Vertices)
            tris.append(m.Triangles + base)
            base += nv
        finally:
            w.close()
    assert np.array_equal(np.concatenate(tris), whole.Triangles)
    assert _eq(np.concatenate(verts), whole.Vertices)


def test_refusals(gpu):
    L = N.lib()
    rng = np.random.default_rng(1)
    plain, _ = _volume(rng, (4, 4, 4), (-1, -1, -1), (1, 1, 1), colors=False)
    h = plain._sync_to_device()
    ops = [(1, -1, -1, -1, -1, 0.0), (2, -1, -1, -1, -1, 0.0), (3, -1, -1, -1, -1, 0.0), (M.NEAREST, 0, 1, 2, 3, 0.0)]

    def create(ops, vols, n=None):
        arr = (N.Op * len(ops))()
        for i, (op, a, b, c, d, imm) in enumerate(ops):
            arr[i].opcode, arr[i].a, arr[i].b, arr[i].c, arr[i].d, arr[i].imm = op, a, b, c, d, imm
        hs = (C.c_void_p * max(len(vols), 1))(*[v.value if v else None for v in vols])
        p = C.c_void_p()
        r = L.sdfk_program_create_bound(arr, len(ops), (C.c_int32 * 4)(-1, -1, -1, len(ops) - 1), 0, hs,
                                        len(vols) if n is None else n, C.byref(p))
        if r == 0:
            L.sdfk_program_destroy(p)
        return r
    assert create(ops, [h]) == 0
    assert create(ops, []) == N.ERR_INVALID                                   # slot 0 of no volume
    assert create(ops[:3] + [(M.NEAREST, 0, 1, 2, (1 << 2) | 3, 0.0)], [h]) == N.ERR_INVALID   # slot 1 of one
    assert create(ops, [h] * 9) == N.ERR_INVALID                              # more than 8
    assert create(ops[:3] + [(M.LINEAR, 0, 1, 2, 1, 0.0)], [h]) == N.ERR_INVALID   # a colour channel of a volume without colours
    assert b"no colours" in L.sdfk_last_error()
    assert create(ops, [None]) == N.ERR_INVALID
    slab = C.c_void_p()
    N.check(L.sdfk_volume_create_slab(4, 4, 8, N.f3((-1, -1, -1)), N.f3((1, 1, 1)), 2, 4, 0, C.byref(slab)))
    assert create(ops, [slab]) == N.ERR_INVALID and b"slab" in L.sdfk_last_error()
    L.sdfk_volume_free(slab)
    flat = C.c_void_p()
    N.check(L.sdfk_volume_create(4, 4, 4, N.f3((-1, -1, 1)), N.f3((1, 1, 1)), 0, C.byref(flat)))
    assert create(ops, [flat]) == N.ERR_INVALID and b"extent" in L.sdfk_last_error()
    L.sdfk_volume_free(flat)
    # the unbound entry point refuses the opcodes
    arr = (N.Op * 4)()
    for i, (op, a, b, c, d, imm) in enumerate(ops):
        arr[i].opcode, arr[i].a, arr[i].b, arr[i].c, arr[i].d, arr[i].imm = op, a, b, c, d, imm
    p = C.c_void_p()
    assert L.sdfk_program_create(arr, 4, (C.c_int32 * 4)(-1, -1, -1, 3), 0, C.byref(p)) == N.ERR_INVALID


def test_node_refuses_volume_programs(gpu):
    from sdfkit_amd import dist as D
    L = N.lib()
    ops = [(1, -1, -1, -1, -1, 0.0), (2, -1, -1, -1, -1, 0.0), (3, -1, -1, -1, -1, 0.0), (M.LINEAR, 0, 1, 2, 3, 0.0)]
    arr = (N.Op * 4)()
    for i, (op, a, b, c, d, imm) in enumerate(ops):
        arr[i].opcode, arr[i].a, arr[i].b, arr[i].c, arr[i].d, arr[i].imm = op, a, b, c, d, imm
    out = (C.c_int32 * 4)(-1, -1, -1, 3)
    with D.Node([0]) as node:
        m = C.c_void_p()
        assert L.sdfk_node_to_mesh(node._h, arr, 4, out, 0, N.f3((-1, -1, -1)), N.f3((1, 1, 1)), 16, 16, 16, 1,
                                   C.c_float(0.0), C.byref(m)) == N.ERR_UNSUPPORTED
        assert not m.value
        nv, ni, hc = C.c_int64(), C.c_int64(), C.c_int32()
        assert L.sdfk_node_mesh_begin(node._h, arr, 4, out, 0, N.f3((-1, -1, -1)), N.f3((1, 1, 1)), 16, 16, 16, 1,
                                      C.c_float(0.0), C.byref(nv), C.byref(ni), C.byref(hc)) == N.ERR_UNSUPPORTED
        # and the node still works
        _, sdf = __import__("tests.scenes", fromlist=["sphere_w"]).sphere_w(1.0)
        assert len(node.to_mesh(sdf, [-1.5] * 3, [1.5] * 3, 24, 24, 24).Vertices) > 0
