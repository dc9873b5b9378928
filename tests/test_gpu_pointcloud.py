"""KdTree.EstimateNormals / ToVoxels on the MI355X against the numpy model (tests/pointcloud_model.py).  Every comparison is bit for
bit: normals, variation and volumes as uint32, stats equal."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from tests import pointcloud_model as PC
from tests import scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [3, 8, 9, 16, 33]           # the register tier at its edge, and the LDS tiers 16 and 64


def _u(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _normals_exact(tree, P, k, viewpoint=None, max_distance=INF):
    nrm, var = tree.EstimateNormals(k, viewpoint, max_distance)
    rn, rv = PC.normals(P, k, viewpoint, max_distance)
    assert nrm.shape == rn.shape and nrm.dtype == f32 and var.dtype == f32
    bad = np.nonzero((_u(nrm) != _u(rn)).any(axis=1) | (_u(var) != _u(rv)))[0]
    assert len(bad) == 0, (k, len(bad), bad[:3], nrm[bad[:3]], rn[bad[:3]], var[bad[:3]], rv[bad[:3]])
    return nrm, var


_cache = {}


def _data(name):
    """name -> (tree, static points, viewpoint, max_distance), made once."""
    if name in _cache:
        return _cache[name]
    rs = np.random.default_rng(31)
    view, md = None, INF
    if name == "uniform":
        P = rs.random((5000, 3), dtype=f32)
    elif name == "mesh":                      # the vertices of a catalogue mesh at 40^3
        _, sdf = S.CATALOGUE["cylinder"]()
        m = sdf.ToMesh([-2.5] * 3, [2.5] * 3, 40, 40, 40, clipToBounds=False)
        P = np.ascontiguousarray(np.asarray(m.Vertices, f32).reshape(-1, 3))
        view = np.array([0.0, 0.0, 0.0], f32)
    elif name == "lattice":                   # mass ties
        g = np.arange(9, dtype=f32)
        P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)
        P = P[rs.permutation(len(P))]
    elif name == "two_batches":
        P = (rs.standard_normal((3000, 3)) * 0.3).astype(f32)
    elif name == "per_point_views":
        P = rs.random((2000, 3), dtype=f32)
        view = (P + rs.standard_normal(P.shape).astype(f32)).astype(f32)
        view[::5] = P[::5]                    # d == 0 exactly
    elif name == "banded":                    # a finite maxDistance that leaves some points with fewer than 3 neighbours
        P = np.concatenate([rs.random((1500, 3), dtype=f32), rs.random((60, 3), dtype=f32) * f32(8) + f32(2)]).astype(f32)
        md = f32(0.12)
    if name == "two_batches":
        tree = K.KdTree(P[:1700])
        tree.AddPoints(P[1700:])
    else:
        tree = K.KdTree(P)
    assert tree.TotalPoints == len(P)
    _cache[name] = (tree, P, view, md)
    return _cache[name]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["uniform", "mesh", "lattice", "two_batches", "per_point_views", "banded"])
def test_normals_equal_the_model(gpu, name, k):
    tree, P, view, md = _data(name)
    nrm, var = _normals_exact(tree, P, k, view, md)
    zero = (nrm == 0).all(axis=1)
    if name == "banded":
        assert zero.any() and not zero.all() and (var[zero] == 0).all()
    else:
        assert not zero.any()
        assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_lattice_plane_and_refusals(gpu):
    g = np.arange(8, dtype=f32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    P = np.stack([X.ravel(), Y.ravel(), np.full(64, 2, f32)], axis=1)
    tree = K.KdTree(P)
    nrm, var = _normals_exact(tree, P, 8)
    assert (nrm == np.array([0, 0, 1], f32)).all() and (var == 0).all()
    nrm, _ = _normals_exact(tree, P, 8, viewpoint=[3, 3, -5])
    assert (nrm == np.array([0, 0, -1], f32)).all()
    for k in (2, 65, 0):
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.EstimateNormals(k)
        assert e.value.status == N.ERR_INVALID
    for bad in dict(maxDistance=np.nan), dict(maxDistance=-1.0), dict(viewpoint=[0, np.inf, 0]), dict(viewpoint=np.zeros((5, 3), f32)):
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.EstimateNormals(8, **bad)
        assert e.value.status == N.ERR_INVALID
    Nn = np.tile(np.array([[0, 0, 1]], f32), (64, 1))
    for bad in dict(k=0), dict(k=65), dict(maxDistance=0.0), dict(maxDistance=np.nan), dict(maxDistance=-2.0):
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.ToVoxels(Nn, [0] * 3, [1] * 3, 4, 4, 4, **bad)
        assert e.value.status == N.ERR_INVALID
    with pytest.raises(ValueError):
        tree.ToVoxels(Nn[:5], [0] * 3, [1] * 3, 4, 4, 4)
    # the plane as a volume: exactly z - 2 (tests/test_pointcloud.py says why these centres)
    v = tree.ToVoxels(Nn, (-0.5, -0.5, 1.5), (7.5, 7.5, 2.5), 16, 16, 2, k=8)
    assert set(np.unique(v.Values)) == {f32(-0.25), f32(0.25)} and (v.Values[:, :, 0] == f32(-0.25)).all()


# ---- volumes ----
def _fibonacci(n):
    i = np.arange(n, dtype=np.float64) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1).astype(f32)


# a sphere cut by the volume's wall at x = -0.4; with a band the corners hold fully unknown columns
BOX = ((-0.4, -1.5, -1.5), (1.5, 1.5, 1.5))
SHAPES = {"odd": (23, 17, 29), "cube": (32, 32, 32)}


@pytest.fixture(scope="module")
def cloud(gpu):
    P = _fibonacci(1200)
    Nn = P.copy()
    Nn[::40] = 0                                  # some points without a normal: skipped
    return K.KdTree(P), P, Nn


@pytest.mark.parametrize("band_voxels", [2, None])
@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("shape", ["odd", "cube"])
def test_volume_equals_the_model(cloud, shape, k, band_voxels):
    tree, P, Nn = cloud
    nx, ny, nz = SHAPES[shape]
    md = INF if band_voxels is None else f32(band_voxels * 3.0 / 32)
    stats = {}
    vox = tree.ToVoxels(Nn, BOX[0], BOX[1], nx, ny, nz, k=k, maxDistance=md, stats=stats)
    want, known = PC.to_volume(P, Nn, BOX[0], BOX[1], (nx, ny, nz), k, md)
    got = vox.Values
    bad = np.argwhere(_u(got) != _u(want))
    assert len(bad) == 0, (len(bad), bad[:3], [(got[tuple(b)], want[tuple(b)], known[tuple(b)]) for b in bad[:3]])
    assert stats["known"] == int(known.sum()) and stats["unknown"] == int((~known).sum())
    if band_voxels is None:
        assert known.all() or k == 1                            # (k = 1: a nearest point without a normal leaves the voxel unknown)
    else:
        assert (~known).all(axis=2).any() and known.any()      # fully unknown columns
        assert (np.abs(got) <= md).all() and (got[~known] < 0).any() and (got[~known] > 0).any()


def test_volume_device_entry_points_give_the_same_bytes(cloud):
    import torch
    tree, P, Nn = cloud
    L = N.lib()
    md = f32(0.2)
    host = tree.ToVoxels(Nn, BOX[0], BOX[1], 23, 17, 29, k=8, maxDistance=md).Values.copy()
    N.bind_torch_stream()
    dev = torch.device("cuda:0")
    Nd = torch.from_numpy(Nn).to(dev)
    vox = K.Voxels(BOX[0], BOX[1], 23, 17, 29)
    h = vox._ensure_device(False)
    st = (C.c_int64 * 4)()
    N.check(L.sdfk_points_to_volume_device(tree.handle, C.c_void_p(Nd.data_ptr()), h, 8, float(md), st))
    N.check(L.sdfk_synchronize())
    vox._host_values = None
    assert np.array_equal(_u(vox.Values), _u(host)) and st[0] + st[1] == 23 * 17 * 29 and 0 < st[0] < 23 * 17 * 29
    # normals: device outputs, one viewpoint on the device
    n = len(P)
    view = torch.tensor([0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    nd = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    vd = torch.zeros(n, dtype=torch.float32, device=dev)
    N.check(L.sdfk_points_normals_device(tree.handle, 12, float(INF), C.c_void_p(view.data_ptr()), 1, C.c_void_p(nd.data_ptr()), C.c_void_p(vd.data_ptr())))
    N.check(L.sdfk_synchronize())
    torch.cuda.synchronize()
    hn, hv = tree.EstimateNormals(12, [0, 0, 0])
    assert np.array_equal(_u(nd.cpu().numpy()), _u(hn)) and np.array_equal(_u(vd.cpu().numpy()), _u(hv))
    assert (np.einsum("ij,ij->i", hn, P) < -0.9).all()          # towards the viewpoint at the centre
    N.check(L.sdfk_set_stream(None))


def test_sample_into_keeps_colours_and_rebinds(gpu):
    tree = K.KdTree(_fibonacci(600))
    Nn = _fibonacci(600)
    vox = K.Voxels([-1.5] * 3, [1.5] * 3, 16, 16, 16)
    vox.Colors[...] = f32(0.25)
    before = vox._version
    assert tree.SampleInto(vox, Nn, 8, 0.5) is vox and vox._version > before
    assert (vox.Colors == f32(0.25)).all() and (vox.Values[8, 8, 8] == f32(-0.5)) and (vox.Values[0, 0, 0] == f32(0.5))


def test_profiled_stats(cloud):
    tree, P, Nn = cloud
    N.check(N.lib().sdfk_profile_enable(1))
    try:
        stats = {}
        tree.ToVoxels(Nn, BOX[0], BOX[1], 8, 8, 8, k=8, maxDistance=0.3, stats=stats)
        assert stats["queries"] == 512 and stats["candidates"] > 0 and tree.stats()["queries"] == 512
        tree.EstimateNormals(8)
        assert tree.stats()["queries"] == len(P) and tree.stats()["candidates"] >= 8 * len(P)
    finally:
        N.check(N.lib().sdfk_profile_enable(0))


def test_round_trip_sphere_mesh_points_volume_redistance_mesh(gpu):
    """Sdfs.Sphere -> mesh -> its vertices and normals as a cloud -> banded volume -> Redistance -> mesh.  The mesher's normals point
    outwards (the gradient of the distance; tests/test_gpu_parity.py asserts it), which is ToVoxels' convention: +mesh.Normals."""
    with open(os.path.join(ROOT, "tests", "golden", "pointcloud_accuracy.json")) as f:
        fig = json.load(f)
    n, h = fig["grid"], 3.0 / fig["grid"]
    _, sdf = S.sphere_w(1.0)
    m = sdf.ToMesh([-1.5] * 3, [1.5] * 3, n, n, n, clipToBounds=False)
    V = np.ascontiguousarray(np.asarray(m.Vertices, f32).reshape(-1, 3))
    Nn = np.ascontiguousarray(np.asarray(m.Normals, f32).reshape(-1, 3))
    assert len(V) >= fig["points"] and (np.einsum("ij,ij->i", Nn, V) > 0).all()
    band = f32(fig["band_voxels"] * h)
    stats = {}
    vox = K.KdTree(V).ToVoxels(Nn, [-1.5] * 3, [1.5] * 3, n, n, n, k=fig["k"], maxDistance=band, stats=stats)
    want, _ = PC.to_volume(V, Nn, [-1.5] * 3, [1.5] * 3, (n, n, n), fig["k"], band)
    assert np.array_equal(_u(vox.Values), _u(want)) and stats["unknown"] > 0
    assert vox.Values[n // 2, n // 2, n // 2] == -band and vox.Values[0, 0, 0] == band
    full = vox.Redistance()
    assert np.isfinite(full.Values).all() and full.Values[n // 2, n // 2, n // 2] < -0.8
    out = full.ToMesh()
    r = np.linalg.norm(np.asarray(out.Vertices, np.float64).reshape(-1, 3), axis=1)
    print("round trip: vertices", len(r), "max |r - 1|", np.abs(r - 1).max(), "bound", fig["roundtrip_vertex_bound"])
    assert len(r) > 0 and np.abs(r - 1).max() <= fig["roundtrip_vertex_bound"]
