"""KdTree.EstimateNormals / ToVoxels on the MI355X on degenerate neighbourhoods and sparse volumes (tests/pointcloud_cases.py)
against the numpy model (tests/pointcloud_model.py): planes, lines, copies, lattices and needles with the search's own tie order, at
the edges of both tiers of k; the same cloud scaled until its d2 are subnormal, huge or zero; viewpoints that are NaN or infinite
(the unchecked device form); sets of one to five points; volumes of thickness 1, and volumes whose lines, slabs or every voxel have
no sign, coloured or not.  Every comparison is bit for bit through uint32 views, and no variation has its sign bit set."""
import ctypes as C

import numpy as np
import pytest

import sdfkit_amd as K
from sdfkit_amd import _native as N
from tests import pointcloud_cases as CS
from tests import pointcloud_color_model as CM
from tests import pointcloud_model as PC
from tests.test_gpu_pointcloud import _normals_exact, _u
from tests.test_pointcloud_cases import SEED, VOLUME_SEED, _views, _volume

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = np.inf
KS = [3, 8, 9, 16, 17, 33, 64]            # the register tier at its edge, and the LDS tiers 16, 32 and 64 at theirs


def _dptr(t):
    return C.c_void_p(t.data_ptr())


def _no_sign_bit(var):
    assert (_u(var) < 0x80000000).all() and (var >= 0).all()


_trees = {}


def _tree(e=0):
    """The cluster cloud times 2^e and its tree, made once."""
    if e not in _trees:
        P = CS.clusters(SEED)[0] if e == 0 else CS.scaled_clusters(SEED, e)[0]
        _trees[e] = (K.KdTree(P), P)
    return _trees[e]


# ---- normals ----
@pytest.mark.parametrize("k", KS)
def test_cluster_normals_equal_the_model(gpu, k):
    tree, P = _tree()
    zero_expected = CS.multiplicity(P) >= k
    for name, view in _views(P).items():
        nrm, var = _normals_exact(tree, P, k, view)
        _no_sign_bit(var)
        zero = (nrm == 0).all(axis=1)
        assert np.array_equal(zero, zero_expected), (name, int(zero.sum()), int(zero_expected.sum()))
        assert (_u(var[zero]) == 0).all() and np.abs(np.linalg.norm(nrm[~zero].astype(np.float64), axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("e,k", [(e, k) for e in (-70, 40) for k in (3, 8, 16, 64)] + [(-140, 8), (-140, 64)])
def test_scaled_cluster_normals_equal_the_model(gpu, e, k):
    tree, S = _tree(e)
    nrm, var = _normals_exact(tree, S, k)
    _no_sign_bit(var)
    assert (nrm != 0).any()
    view = S.copy()
    view[1::5] = S[::-1][1::5]                                    # other points of the cloud as viewpoints; the rest: d == 0
    _no_sign_bit(_normals_exact(tree, S, k, view)[1])


def test_device_form_with_non_finite_viewpoints(gpu):
    """Contract step 7: the _device form does not read the viewpoints on the host; a NaN or infinite one gives a d that is compared
    as it comes (NaN: the rule without viewpoint).  Either output may be NULL, and a second call gives the same bytes."""
    import torch
    tree, P = _tree()
    n = len(P)
    rs = np.random.default_rng(17)
    view = (P + rs.standard_normal(P.shape).astype(f32)).astype(f32)
    view[0::7, 0] = np.nan
    view[1::7] = np.nan
    view[2::7, 1] = np.inf
    view[3::7] = [-np.inf, np.inf, -np.inf]
    view[4::7, 2] = -np.inf
    view[5::7] = P[5::7]
    L = N.lib()
    N.bind_torch_stream()
    dev = torch.device("cuda:0")
    try:
        vd = torch.from_numpy(view).to(dev)
        for k in (8, 33):
            want_n, want_v = PC.normals(P, k, view)
            assert (want_n != PC.normals(P, k)[0]).any()                   # the finite and the infinite ones do turn some
            outs = []
            for _ in range(2):
                nd = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
                wd = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
                N.check(L.sdfk_points_normals_device(tree.handle, k, float(INF), _dptr(vd), n, _dptr(nd), _dptr(wd)))
                N.check(L.sdfk_synchronize())
                torch.cuda.synchronize()
                outs.append((nd.cpu().numpy(), wd.cpu().numpy()))
            (nrm, var), again = outs
            bad = np.nonzero((_u(nrm) != _u(want_n)).any(axis=1) | (_u(var) != _u(want_v)))[0]
            assert len(bad) == 0, (k, len(bad), bad[:3], view[bad[:3]], nrm[bad[:3]], want_n[bad[:3]], var[bad[:3]], want_v[bad[:3]])
            assert np.array_equal(_u(again[0]), _u(nrm)) and np.array_equal(_u(again[1]), _u(var))
            _no_sign_bit(var)
            # either output alone
            nd = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
            wd = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
            N.check(L.sdfk_points_normals_device(tree.handle, k, float(INF), _dptr(vd), n, None, _dptr(wd)))
            N.check(L.sdfk_points_normals_device(tree.handle, k, float(INF), _dptr(vd), n, _dptr(nd), None))
            N.check(L.sdfk_synchronize())
            torch.cuda.synchronize()
            assert np.array_equal(_u(nd.cpu().numpy()), _u(nrm)) and np.array_equal(_u(wd.cpu().numpy()), _u(var))
    finally:
        N.check(L.sdfk_set_stream(None))


def test_tiny_sets(gpu):
    """Fewer points than k: zeros from m < 3, a normal from m = 3 on."""
    P, F = CS.clusters(SEED)
    near = lambda name: P[(F == CS.FAMILY[name]) & (np.abs(P - CS.cluster_centre(name, 0).astype(f32)) <= 0.5).all(axis=1)]
    generic, line = near("generic"), near("collinear_x")
    assert len(generic) == 64 and len(line) == 64
    for S in [generic[:n] for n in (1, 2, 3, 4, 5)] + [line[:3]]:
        tree = K.KdTree(S)
        for k in (3, 64):
            nrm, var = _normals_exact(tree, S, k)
            _no_sign_bit(var)
            assert (nrm == 0).all() == (len(S) < 3) and (len(S) >= 3 or (_u(var) == 0).all())
            view = S[::-1].copy()
            _normals_exact(tree, S, k, view)
    assert (_normals_exact(K.KdTree(line[:3]), line[:3], 3)[0] == np.array([0, 1, 0], f32)).all()


# ---- volumes ----
@pytest.fixture(scope="module")
def sparse(gpu):
    P, Nn = CS.sparse_normal_cloud(VOLUME_SEED)
    return K.KdTree(P), P, Nn


def _volume_exact(vox, stats, want, known):
    got = vox.Values
    assert got.shape == want.shape
    bad = np.argwhere(_u(got) != _u(want))
    assert len(bad) == 0, (len(bad), bad[:3], [(got[tuple(b)], want[tuple(b)], known[tuple(b)]) for b in bad[:3]])
    assert stats["known"] == int(known.sum()) and stats["unknown"] == int((~known).sum())


@pytest.mark.parametrize("shape", CS.VOLUME_SHAPES)
def test_sparse_volumes_equal_the_model(sparse, shape):
    tree, P, Nn = sparse
    for k, md in CS.K_AND_BAND:
        _, _, _, _, known, want = _volume(shape, k, md)
        stats = {}
        vox = tree.ToVoxels(Nn, *CS.BOX, *shape, k=k, maxDistance=md, stats=stats)
        _volume_exact(vox, stats, want, known.reshape(shape))
        if np.isinf(md) and not known.all():
            assert np.isinf(vox.Values).any()


def test_sparse_volume_device_entry_point_and_colours(sparse):
    import torch
    tree, P, Nn = sparse
    shape = (13, 11, 9)
    L = N.lib()
    # the coloured kernel on lines, slabs and voxels without a point
    rs = np.random.default_rng(23)
    col = (rs.standard_normal(P.shape) * 2.0 ** rs.integers(-12, 3, P.shape)).astype(f32)
    for k, md in CS.K_AND_BAND:
        want, known, wcol, found = CM.to_volume(P, Nn, col, *CS.BOX, shape, k, md)
        assert np.array_equal(_u(want), _u(_volume(shape, k, md)[5]))
        stats = {}
        vox = tree.ToVoxels(Nn, *CS.BOX, *shape, k=k, maxDistance=md, stats=stats, colors=col)
        _volume_exact(vox, stats, want, known)
        bad = np.argwhere((_u(vox.Colors) != _u(wcol)).any(axis=3))
        assert len(bad) == 0, (k, md, len(bad), bad[:3])
        if np.isfinite(md):
            assert (found == 0).all(axis=2).any() and (_u(vox.Colors[found == 0]) == 0).all()
    # the _device entry point
    k, md = 8, f32(0.08)
    _, _, _, _, known, want = _volume(shape, 8, 0.08)
    N.bind_torch_stream()
    try:
        Nd = torch.from_numpy(Nn).to(torch.device("cuda:0"))
        vox = K.Voxels(*CS.BOX, *shape)
        h = vox._ensure_device(False)
        st = (C.c_int64 * 4)()
        N.check(L.sdfk_points_to_volume_device(tree.handle, _dptr(Nd), h, k, float(md), st))
        N.check(L.sdfk_synchronize())
        vox._host_values = None
        assert np.array_equal(_u(vox.Values), _u(want)) and st[0] == int(known.sum()) and st[1] == int((~known).sum())
    finally:
        N.check(L.sdfk_set_stream(None))


@pytest.mark.parametrize("k", [1, 8, 64])
def test_cluster_volumes_equal_the_model(gpu, k):
    """Supplied normals over the cluster cloud: cell centres exactly at 64 copies (h2 == 0: the first tangent plane, exactly 0, which
    the fill reads as +), tilted planes, lines and a lattice in the other cells."""
    tree, P = _tree()
    Nn = CS.cluster_normals(SEED)
    assert 0.2 < (Nn == 0).all(axis=1).mean() < 0.4
    for md in (INF, 1.0):
        want, known = PC.to_volume(P, Nn, *CS.CLUSTER_BOX, CS.CLUSTER_SHAPE, k, md)
        stats = {}
        vox = tree.ToVoxels(Nn, *CS.CLUSTER_BOX, *CS.CLUSTER_SHAPE, k=k, maxDistance=md, stats=stats)
        _volume_exact(vox, stats, want, known)
        for cell in CS.COPIES_VOXELS:
            assert known[cell] and vox.Values[cell] == 0
        if np.isfinite(md):
            assert 0 < known.sum() < known.size / 8
