"""Per-point colours through the point-cloud pipeline on the MI355X -- KdTree.SampleColors, ToVoxels / SampleInto(colors=),
VoxelDownsample(colors=) (csrc/lib_pointcloud.hip, csrc/lib_points_filter.hip, csrc/points_color.h) -- against the numpy model
(tests/pointcloud_color_model.py).  Every comparison is bit for bit, as uint32."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from tests import pointcloud_color_model as CM
from tests import scenes as S
from tests.test_gpu_parity import assert_mesh_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 8, 9, 16, 33]            # the register tier at its edge, and the LDS tiers 16 and 64
# a finite maxDistance per cloud and k at which some queries find nothing, some fewer than k and some exactly k (asserted below):
# the radius of a ball that holds about k points of the uniform cloud, a little more than the k-th lattice distance
FINITE = {"uniform": {1: 0.036, 8: 0.0726, 9: 0.0755, 16: 0.0914, 33: 0.1164}, "lattice": {1: 0.4, 8: 1.2, 9: 1.2, 16: 1.5, 33: 2.1}}


def _u(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _dptr(t):
    return C.c_void_p(t.data_ptr())


_cache = {}


def _data(name):
    """name -> (tree, static points, colours, queries), made once."""
    if name in _cache:
        return _cache[name]
    rs = np.random.default_rng(31)
    if name == "uniform":
        P = rs.random((5000, 3), dtype=f32)
        lo, hi = -0.25, 1.25
    else:                                         # "lattice": mass ties
        g = np.arange(9, dtype=f32)
        P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)
        P = P[rs.permutation(len(P))]
        lo, hi = -3.0, 11.0
    col = (rs.standard_normal((len(P), 3)) * 2.0 ** rs.integers(-20, 4, (len(P), 3))).astype(f32)   # sums whose order shows
    col[::13, 2] = -0.0
    Q = np.concatenate([(rs.random((2000, 3), dtype=f32) * f32(hi - lo) + f32(lo)).astype(f32), P,
                        np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5]], f32)])
    _cache[name] = (K.KdTree(P), P, col, Q)
    return _cache[name]


# ---- SampleColors ----
@pytest.mark.parametrize("finite", [False, True])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["uniform", "lattice"])
def test_sample_colors_equal_the_model(gpu, name, k, finite):
    tree, P, col, Q = _data(name)
    md = f32(FINITE[name][k]) if finite else INF
    want, wfound = CM.sample_colors(P, col, Q, k, md)
    got, found = tree.SampleColors(Q, col, k, md)
    assert got.shape == want.shape and got.dtype == f32 and found.dtype == np.int32
    assert np.array_equal(found, wfound)
    bad = np.nonzero((_u(got) != _u(want)).any(axis=1))[0]
    assert len(bad) == 0, (name, k, md, len(bad), bad[:3], got[bad[:3]], want[bad[:3]], found[bad[:3]])
    assert (found[-2:] == 0).all() and (_u(got[-2:]) == 0).all()      # the NaN and the infinite query: nothing, (+0, +0, +0)
    if finite:
        none, short, full = (wfound == 0).sum(), ((wfound > 0) & (wfound < k)).sum(), (wfound == k).sum()
        assert none > 2 and full > 0 and (short > 0 or k == 1), (none, short, full)   # (k = 1 has nothing between 0 and k)
        assert (_u(got[wfound == 0]) == 0).all()
    else:
        assert (wfound[:-2] == k).all()
    if k == 1:                                    # nearest-point colouring, bit for bit
        idx = tree.SearchKNearest(Q, 1, md)[0][:, 0]
        assert np.array_equal(_u(got[idx >= 0]), _u(col[idx[idx >= 0]]))


# ---- coloured volumes ----
def _fibonacci(n):
    i = np.arange(n, dtype=np.float64) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1).astype(f32)


# a sphere cut by the volume's wall at x = -0.4; with a band the corners hold fully unknown columns
BOX = ((-0.4, -1.5, -1.5), (1.5, 1.5, 1.5))
SHAPES = {"odd": (23, 17, 29), "cube": (32, 32, 32)}   # 29 is no multiple of 4: padded rows


@pytest.fixture(scope="module")
def cloud(gpu):
    P = _fibonacci(1200)
    Nn = P.copy()
    Nn[::40] = 0                                  # some points without a normal: skipped by the distances, not by the colours
    rs = np.random.default_rng(77)
    col = np.stack([f32(0.5) + f32(0.25) * P[:, 0], f32(0.5) - f32(0.25) * P[:, 1] * P[:, 2], rs.random(len(P), dtype=f32)], axis=1).astype(f32)
    return K.KdTree(P), P, Nn, col


@pytest.mark.parametrize("band_voxels", [2, None])
@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("shape", ["odd", "cube"])
def test_coloured_volume_equals_the_model(cloud, shape, k, band_voxels):
    tree, P, Nn, col = cloud
    nx, ny, nz = SHAPES[shape]
    md = INF if band_voxels is None else f32(band_voxels * 3.0 / 32)
    stats, plain_stats = {}, {}
    vox = tree.ToVoxels(Nn, BOX[0], BOX[1], nx, ny, nz, k=k, maxDistance=md, stats=stats, colors=col)
    plain = tree.ToVoxels(Nn, BOX[0], BOX[1], nx, ny, nz, k=k, maxDistance=md, stats=plain_stats)
    want, known, wcol, found = CM.to_volume(P, Nn, col, BOX[0], BOX[1], (nx, ny, nz), k, md)
    got, gcol = vox.Values, vox.Colors
    bad = np.argwhere(_u(got) != _u(want))
    assert len(bad) == 0, (len(bad), bad[:3], [(got[tuple(b)], want[tuple(b)], known[tuple(b)]) for b in bad[:3]])
    bad = np.argwhere((_u(gcol) != _u(wcol)).any(axis=3))
    assert len(bad) == 0, (len(bad), bad[:3], [(gcol[tuple(b)], wcol[tuple(b)], found[tuple(b)]) for b in bad[:3]])
    # the distances are the colourless call's, and so are the stats
    assert np.array_equal(_u(got), _u(plain.Values)) and stats == plain_stats
    assert stats["known"] == int(known.sum()) and stats["unknown"] == int((~known).sum())
    assert not plain.Colors.any()
    # a colour wherever a point was found -- also where every neighbour lacks a normal and the distance is unknown
    orphan = (found > 0) & ~known
    print("coloured volume", shape, k, band_voxels, "found nothing", int((found == 0).sum()), "colour without a value", int(orphan.sum()))
    assert gcol[orphan].any() == bool(orphan.any())
    if band_voxels is None:
        assert (found > 0).all()
    else:
        assert (found == 0).any() and (_u(gcol[found == 0]) == 0).all()      # no point within the band: zero colours
        if k == 1:
            assert orphan.any()


def test_colour_device_entry_points_give_the_same_bytes(cloud):
    import torch
    tree, P, Nn, col = cloud
    L = N.lib()
    md = f32(0.2)
    n = len(P)
    host = tree.ToVoxels(Nn, BOX[0], BOX[1], 23, 17, 29, k=8, maxDistance=md, colors=col)
    hv, hc = host.Values.copy(), host.Colors.copy()
    Q = np.concatenate([P[:100], (P * f32(1.1)).astype(f32)])
    hq, hf = tree.SampleColors(Q, col, 12, md)
    hd = tree.VoxelDownsample(0.25, colors=col)
    N.bind_torch_stream()
    dev = torch.device("cuda:0")
    Nd, Cd, Qd = (torch.from_numpy(a).to(dev) for a in (Nn, col, Q))
    try:
        vox = K.Voxels(BOX[0], BOX[1], 23, 17, 29)
        h = vox._ensure_device(True)
        st = (C.c_int64 * 4)()
        N.check(L.sdfk_points_to_volume_colors_device(tree.handle, _dptr(Nd), _dptr(Cd), h, 8, float(md), st))
        N.check(L.sdfk_synchronize())
        vox._host_values = vox._host_colors = None
        assert np.array_equal(_u(vox.Values), _u(hv)) and np.array_equal(_u(vox.Colors), _u(hc))
        assert st[0] + st[1] == 23 * 17 * 29 and 0 < st[0] < 23 * 17 * 29
        # colours at queries
        od = torch.full((len(Q), 3), -7.0, dtype=torch.float32, device=dev)
        fd = torch.full((len(Q),), -7, dtype=torch.int32, device=dev)
        N.check(L.sdfk_points_blend_colors_device(tree.handle, _dptr(Cd), _dptr(Qd), len(Q), 12, float(md), _dptr(od), _dptr(fd)))
        N.check(L.sdfk_synchronize())
        torch.cuda.synchronize()
        assert np.array_equal(_u(od.cpu().numpy()), _u(hq)) and np.array_equal(fd.cpu().numpy(), hf)
        # either output may be left out
        N.check(L.sdfk_points_blend_colors_device(tree.handle, _dptr(Cd), _dptr(Qd), len(Q), 12, float(md), None, _dptr(fd)))
        N.check(L.sdfk_points_blend_colors_device(tree.handle, _dptr(Cd), _dptr(Qd), len(Q), 12, float(md), _dptr(od), None))
        N.check(L.sdfk_synchronize())
        assert np.array_equal(_u(od.cpu().numpy()), _u(hq)) and np.array_equal(fd.cpu().numpy(), hf)
        # the filter
        pts = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
        out = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
        cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
        grp = torch.full((n,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        m = C.c_int64(-1)
        o = (C.c_float * 3)(0, 0, 0)
        N.check(L.sdfk_points_voxel_downsample_colors_device(tree.handle, 0.25, o, _dptr(Cd), _dptr(pts), _dptr(cnt), _dptr(grp), _dptr(out), C.byref(m)))
        pts, out, cnt, grp = (t.cpu().numpy() for t in (pts, out, cnt, grp))       # (the call has finished when it returns)
        assert m.value == len(hd[0]) and (out[m.value:] == -7).all() and (pts[m.value:] == -7).all()   # entries from m on are left alone
        assert np.array_equal(_u(pts[:m.value]), _u(hd[0])) and np.array_equal(cnt[:m.value], hd[1]) and np.array_equal(grp, hd[2])
        assert np.array_equal(_u(out[:m.value]), _u(hd[3]))
    finally:
        N.check(L.sdfk_set_stream(None))


def test_sample_into_with_and_without_colours(cloud):
    tree, P, Nn, col = cloud
    L = N.lib()
    box = ([-1.5] * 3, [1.5] * 3, 16, 16, 16)
    want, _, wcol, found = CM.to_volume(P, Nn, col, box[0], box[1], (16, 16, 16), 8, 0.5)
    # colours that were there are overwritten
    vox = K.Voxels(*box)
    vox.Colors[...] = f32(0.25)
    vox.Values[...] = f32(3)
    before = vox._version
    assert tree.SampleInto(vox, Nn, 8, 0.5, colors=col) is vox and vox._version > before
    assert np.array_equal(_u(vox.Values), _u(want)) and np.array_equal(_u(vox.Colors), _u(wcol)) and (found == 0).any()
    # ... and without colours the same call leaves them alone
    assert tree.SampleInto(vox, Nn, 1, 0.5) is vox
    assert np.array_equal(_u(vox.Colors), _u(wcol)) and not np.array_equal(_u(vox.Values), _u(want))
    vox = K.Voxels(*box)
    vox.Colors[...] = f32(0.25)
    tree.SampleInto(vox, Nn, 8, 0.5)
    assert (vox.Colors == f32(0.25)).all() and np.array_equal(_u(vox.Values), _u(want))
    # a volume whose device copy has no colour storage gets it through the Python layer
    vox = tree.ToVoxels(Nn, box[0], box[1], 16, 16, 16, k=8, maxDistance=0.5)
    assert not vox._has_colors
    tree.SampleInto(vox, Nn, 8, 0.5, colors=col)
    assert vox._has_colors and np.array_equal(_u(vox.Values), _u(want)) and np.array_equal(_u(vox.Colors), _u(wcol))
    # the raw entry point refuses a colourless volume, and leaves it as it is
    bare = tree.ToVoxels(Nn, box[0], box[1], 16, 16, 16, k=8, maxDistance=0.5)
    assert L.sdfk_points_to_volume_colors(tree.handle, _ptr(Nn), _ptr(col), bare._h, 8, 0.5, None) == N.ERR_INVALID
    assert b"colours" in L.sdfk_last_error()
    assert np.array_equal(_u(bare.Values), _u(want))


def test_colour_refusals(cloud):
    tree, P, Nn, col = cloud
    L = N.lib()
    Q = P[:5]
    for bad in dict(k=0), dict(k=65), dict(maxDistance=np.nan), dict(maxDistance=-1.0):
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.SampleColors(Q, col, **bad)
        assert e.value.status == N.ERR_INVALID
    for bad in dict(k=0), dict(k=65), dict(maxDistance=np.nan), dict(maxDistance=-2.0), dict(maxDistance=0.0):
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.ToVoxels(Nn, [0] * 3, [1] * 3, 4, 4, 4, colors=col, **bad)
        assert e.value.status == N.ERR_INVALID
    with pytest.raises(N.SdfKitNativeError) as e:
        tree.VoxelDownsample(0.0, colors=col)
    assert e.value.status == N.ERR_INVALID
    # one colour per static point
    with pytest.raises(ValueError):
        tree.SampleColors(Q, col[:7])
    with pytest.raises(ValueError):
        tree.ToVoxels(Nn, [0] * 3, [1] * 3, 4, 4, 4, colors=col[:7])
    with pytest.raises(ValueError):
        tree.VoxelDownsample(0.25, colors=col[:7])
    # NULL colours, NULL set
    out = np.full((5, 3), -7, f32)
    vox = K.Voxels([0] * 3, [1] * 3, 4, 4, 4)
    h = vox._ensure_device(True)
    m = C.c_int64(-1)
    assert L.sdfk_points_blend_colors(tree.handle, None, _ptr(Q), 5, 8, INF, _ptr(out), None) == N.ERR_INVALID
    assert L.sdfk_points_blend_colors(None, _ptr(col), _ptr(Q), 5, 8, INF, _ptr(out), None) == N.ERR_INVALID
    assert L.sdfk_points_to_volume_colors(tree.handle, _ptr(Nn), None, h, 8, INF, None) == N.ERR_INVALID
    assert L.sdfk_points_voxel_downsample_colors(tree.handle, 0.25, None, None, _ptr(out), None, None, _ptr(out), C.byref(m)) == N.ERR_INVALID
    assert (out == -7).all() and m.value == -1
    # no queries: nothing to do, still checked
    got, found = tree.SampleColors(np.zeros((0, 3), f32), col)
    assert got.shape == (0, 3) and found.shape == (0,)


# ---- the filter ----
def test_downsample_colours_equal_the_model(gpu):
    """Voxels of 1, 32, 33 and 100 members -- one chunk short, one full, one chunk and a member, four chunks -- built by stacking
    jittered copies of the voxel centres of a 4^3 lattice, in random order over more than one tile of the sort."""
    rs = np.random.default_rng(9)
    g = np.arange(4, dtype=f32) + f32(0.5)
    centres = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    copies = np.array([1, 32, 33, 100])[np.arange(64) % 4]
    P = np.repeat(centres, copies, axis=0)
    P = (P + (rs.random(P.shape) - 0.5) * 0.8).astype(f32)
    P = P[rs.permutation(len(P))]
    col = (rs.standard_normal(P.shape) * 2.0 ** rs.integers(-40, 1, P.shape)).astype(f32)          # sums whose order shows
    tree = K.KdTree(P)
    pts, cnt, grp, out = tree.VoxelDownsample(1.0, colors=col)
    assert np.array_equal(np.bincount(cnt, minlength=101)[[1, 32, 33, 100]], [16, 16, 16, 16]) and len(cnt) == 64
    wp, wc, wg, wout = CM.voxel_downsample(P, col, 1.0)
    assert np.array_equal(_u(out), _u(wout))
    assert np.array_equal(_u(pts), _u(wp)) and np.array_equal(cnt, wc) and np.array_equal(grp, wg)
    # the first three outputs are the colourless call's
    p0, c0, g0 = tree.VoxelDownsample(1.0)
    assert np.array_equal(_u(pts), _u(p0)) and np.array_equal(cnt, c0) and np.array_equal(grp, g0)
    # averaging the points themselves is the centroid
    assert np.array_equal(_u(tree.VoxelDownsample(1.0, colors=P)[3]), _u(pts))
    # below the spacing: the colours in order; a channel of -0.0 comes back as +0.0, as a coordinate does
    col[::3, 1] = -0.0
    pts, cnt, grp, out = tree.VoxelDownsample(1e-5, colors=col)
    assert (cnt == 1).all() and np.array_equal(grp, np.arange(len(P)))
    assert np.array_equal(_u(out), _u(CM.voxel_downsample(P, col, 1e-5)[3]))
    assert (_u(out[::3, 1]) == 0).all() and np.array_equal(_u(out[:, [0, 2]]), _u(col[:, [0, 2]]))
    assert np.array_equal(_u(out[:, 1]), _u(np.where(col[:, 1] == 0, f32(0), col[:, 1])))


# ---- end to end ----
def test_coloured_sphere_cloud_to_coloured_mesh(gpu):
    """Sdfs.Sphere -> mesh -> its vertices and normals as a cloud coloured 0.5 + 0.25 p -> coloured banded volume -> mesh.  The mesh
    equals the oracle's mesh of the model's volume bit for bit, so its colour error is the recorded one, without margin."""
    with open(os.path.join(ROOT, "tests", "golden", "pointcloud_accuracy.json")) as f:
        fig = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "pointcloud_color_accuracy.json")) as f:
        rec = json.load(f)
    e = CM.end_to_end(fig)
    n = fig["grid"]
    _, sdf = S.sphere_w(1.0)
    m = sdf.ToMesh([-1.5] * 3, [1.5] * 3, n, n, n, clipToBounds=False)
    V = np.ascontiguousarray(np.asarray(m.Vertices, f32).reshape(-1, 3))
    Nn = np.ascontiguousarray(np.asarray(m.Normals, f32).reshape(-1, 3))
    assert np.array_equal(_u(V), _u(e["points"])) and np.array_equal(_u(Nn), _u(e["normals"])) and len(V) == rec["cloud_points"]
    col = (f32(0.5) + f32(0.25) * V).astype(f32)
    assert np.array_equal(_u(col), _u(e["colors"]))
    vox = K.KdTree(V).ToVoxels(Nn, [-1.5] * 3, [1.5] * 3, n, n, n, k=fig["k"], maxDistance=e["band"], colors=col)
    assert np.array_equal(_u(vox.Values), _u(e["values"])) and np.array_equal(_u(vox.Colors), _u(e["volume_colors"]))
    out = vox.ToMesh()
    assert_mesh_equal(out, e["mesh"])
    assert len(out.Vertices) == rec["mesh_vertices"] > 0
    err = float(np.abs(np.asarray(out.Colors, np.float64).reshape(-1, 3) - (0.5 + 0.25 * np.asarray(out.Vertices, np.float64).reshape(-1, 3))).max())
    print("coloured round trip: vertices", len(out.Vertices), "max colour error", err, "recorded", rec["vertex_color_error_max"])
    assert err <= rec["vertex_color_error_max"]
    # Redistance copies the colours
    full = vox.Redistance()
    assert np.array_equal(_u(full.Colors), _u(vox.Colors)) and np.isfinite(full.Values).all()
