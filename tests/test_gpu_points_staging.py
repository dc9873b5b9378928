"""What the staging of the point-cloud and volume entry points (csrc/device_stage.h under lib_points*.hip, lib_orient.hip,
lib_pointcloud.hip, lib_redistance.hip, lib_volume.hip) must keep, in one place: an optional output left null changes no other
output; a compacted output is written up to its count and no further; a host form writes the bytes its device form writes;
`stats` null or given changes nothing else; a refusal leaves everything as it was; the arrays a set adopts outlive the call that
made them.  Through the ctypes table of sdfkit_amd/_native.py, with the helpers of tests/test_gpu_mesh_staging.py.

The cloud: 300 points near the unit sphere with colours, the first 20 once more (exact duplicates: a voxel downsample yields
m < n), and five far points, far from each other too (the outlier rule drops them: 0 < kept < n).  The volume is 9 x 10 x 11
with colours: nz % 4 != 0, so rows are padded and upload / download go through the repitch path.  Staging goes wrong in the
pointer and length bookkeeping, not at scale: everything is compared byte for byte, canaries included."""
import ctypes as C

import numpy as np
import pytest

from sdfkit_amd import _native as N
from tests.test_gpu_mesh_staging import CANARY, _Scalars, _call, _vp

pytestmark = pytest.mark.gpu
f32, i32, i64, u8 = np.float32, np.int32, np.int64, np.uint8
INF = float("inf")
fl = C.c_float


def _cloud():
    rng = np.random.default_rng(11)
    d = rng.normal(size=(300, 3))
    sphere = (d / np.linalg.norm(d, axis=1, keepdims=True) * (1.0 + 0.01 * rng.normal(size=(300, 1)))).astype(f32)
    far = np.array([(10, 0, 0), (0, 12, 0), (0, 0, -11), (-9, 9, 0), (8, -8, 8)], f32)
    P = np.ascontiguousarray(np.concatenate([sphere, sphere[:20], far]))
    nrm = (P / np.linalg.norm(P, axis=1, keepdims=True)).astype(f32)
    return P, rng.random(P.shape).astype(f32), np.ascontiguousarray(nrm), rng


POINTS, COLORS, NORMALS, _rng = _cloud()
NP = len(POINTS)
FLIPPED = np.ascontiguousarray(NORMALS * np.where(_rng.random((NP, 1)) < 0.4, -1, 1).astype(f32))   # (orientation has something to flip)
QUERIES = np.ascontiguousarray(np.concatenate([_rng.uniform(-1.5, 1.5, (40, 3)).astype(f32), POINTS[::50]]))
NQ = len(QUERIES)
_c, _s = np.cos(0.3), np.sin(0.3)
DYNAMIC = np.ascontiguousarray((POINTS[:150] @ np.array([[_c, -_s, 0], [_s, _c, 0], [0, 0, 1]]).T + (0.1, -0.05, 0.02)).astype(f32))

DIMS, MN, MX = (9, 10, 11), [-1.5] * 3, [1.5] * 3
_axes = [MN[a] + (np.arange(DIMS[a]) + 0.5) * (MX[a] - MN[a]) / DIMS[a] for a in range(3)]
VALUES = np.ascontiguousarray((np.sqrt(sum(g * g for g in np.meshgrid(*_axes, indexing="ij"))) - 0.9).astype(f32))   # a sphere; z fastest
VCOLORS = _rng.random(DIMS + (3,)).astype(f32)


class _Null:
    """A null `stats` in the place of the int64 outputs of a call, after the `leading` ones (which the caller keeps)."""

    def __init__(self, *leading):
        self.leading = list(leading)

    def args(self):
        return self.leading + [None]

    def values(self):
        return []


class _IcpTail:
    """What follows the points in sdfk_icp_register*: n, total[16], iterations and, for the plane metric, stats[4]."""

    def __init__(self, n, plane):
        self.n, self.total, self.iters = n, (fl * 16)(*[CANARY] * 16), C.c_int32(-CANARY)
        self.stats = [(C.c_int64 * 4)(*[-CANARY] * 4)] if plane else []

    def args(self):
        return [self.n, self.total, C.byref(self.iters)] + self.stats

    def values(self):
        return [list(self.total), self.iters.value] + [list(s) for s in self.stats]


def _points(P, device=False):
    h = C.c_void_p()
    _call("sdfk_points_create", [P, len(P), C.byref(h)], [], _Scalars(), device=device)
    return h


@pytest.fixture(scope="module")
def cloud(gpu):
    h = _points(POINTS)
    yield h
    N.lib().sdfk_points_free(h)


def _volume(colors, values=None, vcolors=None):
    v = C.c_void_p()
    N.check(N.lib().sdfk_volume_create(*DIMS, N.f3(MN), N.f3(MX), 1 if colors else 0, C.byref(v)))
    if values is not None:
        N.check(N.lib().sdfk_volume_upload(v, _vp(values), _vp(vcolors) if colors else None))
    return v


def _download(v, colors):
    vals, cols = np.full(DIMS, CANARY, f32), np.full(DIMS + (3,), CANARY, f32)
    N.check(N.lib().sdfk_volume_download(v, _vp(vals), _vp(cols) if colors else None))
    return vals.tobytes(), cols.tobytes()


def _entries(cloud):
    """name -> (pre, outs, scalar lengths) of every entry point with optional outputs."""
    return {
        "sdfk_points_search": ([cloud, QUERIES, NQ], [(i32, (NQ,)), (f32, (NQ,)), (f32, (NQ, 3))], ()),
        "sdfk_points_knn": ([cloud, QUERIES, NQ, 5, fl(0.8)], [(i32, (NQ, 5)), (f32, (NQ, 5)), (i32, (NQ,))], ()),
        "sdfk_points_normals": ([cloud, 8, fl(INF), None, 0], [(f32, (NP, 3)), (f32, (NP,))], ()),
        "sdfk_points_voxel_downsample": ([cloud, fl(0.25), None], [(f32, (NP, 3)), (i32, (NP,)), (i32, (NP,))], (0,)),
        "sdfk_points_voxel_downsample_colors": ([cloud, fl(0.25), None, COLORS], [(f32, (NP, 3)), (i32, (NP,)), (i32, (NP,)), (f32, (NP, 3))], (0,)),
        "sdfk_points_outliers": ([cloud, 8, fl(1.0), fl(INF)], [(f32, (NP,)), (u8, (NP,)), (i32, (NP,)), (f32, (NP, 3))], (0, 6)),
    }


ENTRIES = ["sdfk_points_search", "sdfk_points_knn", "sdfk_points_normals", "sdfk_points_voxel_downsample", "sdfk_points_voxel_downsample_colors",
           "sdfk_points_outliers"]


@pytest.mark.parametrize("name", ENTRIES)
def test_an_optional_output_alone_equals_it_among_all(cloud, name):
    pre, outs, lengths = _entries(cloud)[name]
    full, counts = _call(name, pre, outs, _Scalars(*lengths))
    assert not any(np.all(a == CANARY) for a in full), name          # (every output was written)
    for k in range(len(outs)):
        lone, lone_counts = _call(name, pre, outs, _Scalars(*lengths), only=k)
        assert lone[k].tobytes() == full[k].tobytes(), (name, k)
        assert lone_counts == counts, (name, k)
    none, none_counts = _call(name, pre, outs, _Scalars(*lengths), only=-1)   # (nothing asked for: not an error, the same counts)
    assert none_counts == counts, name


def test_compacted_outputs_stop_at_their_counts(cloud):
    pre, outs, lengths = _entries(cloud)["sdfk_points_voxel_downsample_colors"]
    (pts, counts, group, cols), (m,) = _call("sdfk_points_voxel_downsample_colors", pre, outs, _Scalars(*lengths))
    assert 8 < m < NP                                                             # (the precondition: duplicates share a voxel)
    for a in (pts, counts, cols):
        assert np.all(a[m:] == CANARY) and not np.all(a[:m] == CANARY)
    assert counts[:m].min() >= 1 and counts[:m].sum() == NP
    assert group.min() == 0 and group.max() == m - 1 and len(np.unique(group)) == m          # (written whole: it is not compacted)
    assert np.array_equal(np.bincount(group, minlength=m), counts[:m])
    (pts2, counts2, group2), (m2,) = _call("sdfk_points_voxel_downsample", *_entries(cloud)["sdfk_points_voxel_downsample"][:2], _Scalars(0))
    assert m2 == m and (pts2.tobytes(), counts2.tobytes(), group2.tobytes()) == (pts.tobytes(), counts.tobytes(), group.tobytes())
    pre, outs, lengths = _entries(cloud)["sdfk_points_outliers"]
    (mean, keep, index, kept_pts), (kept, stats) = _call("sdfk_points_outliers", pre, outs, _Scalars(*lengths))
    assert 0 < kept < NP and stats[0] == kept and stats[0] + stats[1] + stats[2] == NP     # (the precondition: the far points go)
    assert np.all(index[kept:] == CANARY) and np.all(kept_pts[kept:] == CANARY)
    assert set(np.unique(keep)) == {0, 1} and keep.sum() == kept and not np.any(mean == CANARY)   # (written whole)
    assert np.array_equal(index[:kept], np.flatnonzero(keep)) and np.array_equal(kept_pts[:kept], POINTS[keep == 1])
    assert not np.any(keep[-5:])                                                  # (the five far points)


def test_host_forms_write_what_device_forms_write(cloud):
    entries = {name: (name,) + e for name, e in _entries(cloud).items()}
    entries.update({
        "orient": ("sdfk_points_orient_normals", [cloud, 8, fl(INF), 16], [(f32, FLIPPED)], (9,)),
        "blend": ("sdfk_points_blend_colors", [cloud, COLORS, QUERIES, NQ, 6, fl(0.9)], [(f32, (NQ, 3)), (i32, (NQ,))], ()),
    })
    for what, (name, pre, outs, lengths) in entries.items():
        host, host_counts = _call(name, pre, outs, _Scalars(*lengths))
        dev, dev_counts = _call(name, pre, outs, _Scalars(*lengths), device=True)
        assert host_counts == dev_counts, what
        for k, (a, b) in enumerate(zip(host, dev)):
            assert a.tobytes() == b.tobytes(), (what, k)     # (canaries beyond the counts included)
        assert not any(np.all(a == CANARY) for a in host), what
    flipped = _call("sdfk_points_orient_normals", *entries["orient"][1:3], _Scalars(9))
    assert flipped[1][0][2] > 0 and flipped[0][0].tobytes() != FLIPPED.tobytes()          # (stats[2]: some normals were flipped)


@pytest.mark.parametrize("colors", [False, True])
def test_to_volume_host_equals_device_and_stats_change_nothing(cloud, colors):
    name = "sdfk_points_to_volume_colors" if colors else "sdfk_points_to_volume"
    got = {}
    for device in (False, True):
        for scalars in (_Scalars(4), _Null()):
            v = _volume(True, np.zeros(DIMS, f32), VCOLORS)
            _, st = _call(name, [cloud, NORMALS] + ([COLORS] if colors else []) + [v, 8, fl(0.6)], [], scalars, device=device)
            got[device, bool(st)] = _download(v, True)
            N.lib().sdfk_volume_free(v)
            if st:
                assert 0 < st[0][0] < np.prod(DIMS) and st[0][0] + st[0][1] == np.prod(DIMS), st      # (known + filled = all)
                got["stats", device] = st
    assert len(set(got[d, s] for d in (False, True) for s in (False, True))) == 1
    assert got["stats", False] == got["stats", True]
    values, vcolors = got[False, True]
    assert not np.any(np.frombuffer(values, f32) == 0) and (vcolors != VCOLORS.tobytes()) == colors   # (the colourless call leaves the colours)


@pytest.mark.parametrize("plane", [False, True])
def test_icp_host_equals_device_on_both_sides_of_a_chunk(cloud, plane):
    name = "sdfk_icp_register_plane" if plane else "sdfk_icp_register"
    identity = [1.0 if q % 5 == 0 else 0.0 for q in range(16)]
    for iterations in (0, 1, 4, 5):   # (the host reads the stop flag every 4 iterations)
        prm = N.IcpParams(iterations, 0.05, 0.0, 0.0)   # (thresholds of zero: no early convergence)
        pre = [cloud, C.byref(prm)] + ([NORMALS] if plane else [])
        (host,), hv = _call(name, pre, [(f32, DYNAMIC)], _IcpTail(len(DYNAMIC), plane))
        (dev,), dv = _call(name, pre, [(f32, DYNAMIC)], _IcpTail(len(DYNAMIC), plane), device=True)
        assert host.tobytes() == dev.tobytes() and hv == dv, iterations
        assert hv[1] == iterations, hv
        if iterations == 0:
            assert hv[0] == identity and host.tobytes() == DYNAMIC.tobytes()
        else:
            assert hv[0] != identity and host.tobytes() != DYNAMIC.tobytes() and CANARY not in hv[0]


def test_outliers_and_orientation_with_and_without_stats(cloud):
    pre, outs, _ = _entries(cloud)["sdfk_points_outliers"]
    with_stats, (kept, _) = _call("sdfk_points_outliers", pre, outs, _Scalars(0, 6))
    kept_alone = C.c_int64(-CANARY)
    without, _ = _call("sdfk_points_outliers", pre, outs, _Null(C.byref(kept_alone)))
    assert kept_alone.value == kept and [a.tobytes() for a in without] == [a.tobytes() for a in with_stats]
    neither, _ = _call("sdfk_points_outliers", pre, outs, _Null(None))            # (n_kept null as well)
    assert [a.tobytes() for a in neither] == [a.tobytes() for a in with_stats]
    a, _ = _call("sdfk_points_orient_normals", [cloud, 8, fl(INF), 16], [(f32, FLIPPED)], _Scalars(9))
    b, _ = _call("sdfk_points_orient_normals", [cloud, 8, fl(INF), 16], [(f32, FLIPPED)], _Null())
    assert a[0].tobytes() == b[0].tobytes()


@pytest.mark.parametrize("colors", [False, True])
@pytest.mark.parametrize("in_place", [False, True])
def test_redistance_with_and_without_stats(gpu, colors, in_place):
    L, got = N.lib(), []
    for stats in ((C.c_int64 * 4)(*[-CANARY] * 4), None):
        src = _volume(colors, VALUES, VCOLORS)
        dst = src if in_place else _volume(colors, np.zeros(DIMS, f32), np.zeros(DIMS + (3,), f32))
        N.check(L.sdfk_volume_redistance(src, dst, 0.0, INF, stats))
        got.append(_download(dst, colors))
        if not in_place:
            assert _download(src, colors) == (VALUES.tobytes(), VCOLORS.tobytes() if colors else got[-1][1])
            L.sdfk_volume_free(dst)
        L.sdfk_volume_free(src)
        if stats is not None:
            assert stats[0] > 0 and stats[2] > 0 and -CANARY not in list(stats), list(stats)   # (sweeps, front voxels)
    assert got[0] == got[1]
    assert got[0][0] != VALUES.tobytes() and (not colors or got[0][1] == VCOLORS.tobytes())     # (redistanced; the colours carried over)


def test_a_refusal_leaves_everything_as_it_was(gpu):
    L = N.lib()
    # a NaN point is not added: the set, its count and what a search answers stay
    for device in (False, True):
        h = _points(POINTS, device)
        before, _ = _call("sdfk_points_search", [h, QUERIES, NQ], [(i32, (NQ,)), (f32, (NQ,)), (f32, (NQ, 3))], _Scalars())
        bad = np.array([(0.5, 0.5, 0.5), (np.nan, 0, 0)], f32)
        with pytest.raises(N.SdfKitNativeError, match="NaN or infinite"):
            _call("sdfk_points_add", [h, bad, 2], [], _Scalars(), device=device)
        n = C.c_int64()
        N.check(L.sdfk_points_count(h, C.byref(n)))
        after, _ = _call("sdfk_points_search", [h, QUERIES, NQ], [(i32, (NQ,)), (f32, (NQ,)), (f32, (NQ, 3))], _Scalars())
        assert n.value == NP and [a.tobytes() for a in after] == [a.tobytes() for a in before]
        L.sdfk_points_free(h)
    # an infinite point makes no set
    h = C.c_void_p(1)
    bad = POINTS.copy()
    bad[NP // 2, 1] = np.inf
    assert L.sdfk_points_create(_vp(bad), NP, C.byref(h)) == N.ERR_INVALID and h.value is None
    # a volume holding a NaN is not redistanced: dst and stats stay
    bad = VALUES.copy()
    bad[4, 5, 6] = np.nan
    src, dst = _volume(True, bad, VCOLORS), _volume(True, VALUES, VCOLORS)
    stats = (C.c_int64 * 4)(*[-CANARY] * 4)
    assert L.sdfk_volume_redistance(src, dst, 0.0, INF, stats) == N.ERR_INVALID and b"NaN or infinite" in L.sdfk_last_error()
    assert _download(dst, True) == (VALUES.tobytes(), VCOLORS.tobytes()) and list(stats) == [-CANARY] * 4
    L.sdfk_volume_free(src)
    L.sdfk_volume_free(dst)


def test_what_a_set_adopts_outlives_the_call_that_made_it(cloud):
    """The arrays of a build are the set's afterwards: other calls' scratch comes and goes on the same pool in between."""
    L = N.lib()
    search = lambda h: [a.tobytes() for a in _call("sdfk_points_search", [h, QUERIES, NQ], [(i32, (NQ,)), (f32, (NQ,)), (f32, (NQ, 3))], _Scalars())[0]]
    want = search(cloud)
    for device in (False, True):
        h = _points(POINTS[:100], device)
        _call("sdfk_points_add", [h, POINTS[100:], NP - 100], [], _Scalars(), device=device)
        pre, outs, lengths = _entries(h)["sdfk_points_outliers"]
        _call("sdfk_points_outliers", pre, outs, _Scalars(*lengths))
        _call("sdfk_points_voxel_downsample", *_entries(h)["sdfk_points_voxel_downsample"][:2], _Scalars(0))
        assert search(h) == want, device
        L.sdfk_points_free(h)


def test_upload_download_and_eval_on_the_pitched_volume(gpu):
    import sdfkit_amd as K
    L = N.lib()
    for colors in (False, True):
        v, pitch = _volume(colors, VALUES, VCOLORS), C.c_int32()
        N.check(L.sdfk_volume_row_pitch(v, C.byref(pitch)))
        assert pitch.value != DIMS[2]                                             # (the precondition: rows are padded)
        values, vcolors = _download(v, colors)
        assert values == VALUES.tobytes() and (not colors or vcolors == VCOLORS.tobytes())
        L.sdfk_volume_free(v)
    rgbw = _rng.random((NQ, 4)).astype(f32)
    for sdf, writes in ((K.SdfExprs.Sphere(0.5, (0.2, 0.5, 0.9)).ToSdf(), True), (K.Sdfs.Sphere(0.5), False)):
        (host,), _ = _call("sdfk_eval_points", [sdf.program(), QUERIES, NQ], [(f32, rgbw)], _Scalars())
        (dev,), _ = _call("sdfk_eval_points", [sdf.program(), QUERIES, NQ], [(f32, rgbw)], _Scalars(), device=True)
        assert host.tobytes() == dev.tobytes()
        assert np.allclose(host[:, 3], np.linalg.norm(QUERIES.astype(np.float64), axis=1) - 0.5, atol=1e-5)   # (the distance was written)
        if writes:
            assert np.all(host[:, :3] == np.array([0.2, 0.5, 0.9], f32))
        else:
            assert host[:, :3].tobytes() == rgbw[:, :3].tobytes()                 # (a program without colour leaves the caller's)


def test_raymarch_each_image_alone_equals_it_in_the_pair(gpu):
    import sdfkit_amd as K
    w, h = 8, 6
    sdf = K.SdfExprs.Sphere(0.5, (0.2, 0.5, 0.9)).ToSdf()
    rm = K.RayMarcher(w, h, sdf)
    rm.ViewTransform = K.Matrix4x4.CreateLookAt((0, 0, 3), (0, 0, 0), (0, 1, 0))
    pos, vpi = rm.camera()
    pre = [sdf.program(), w, h, N.f3(pos), (fl * 16)(*[float(x) for x in vpi.ravel()]), fl(rm.NearPlaneDistance), fl(rm.FarPlaneDistance), 32]
    outs = [(f32, (h, w)), (f32, (h, w, 3))]
    both, _ = _call("sdfk_raymarch", pre, outs, _Scalars())
    assert not np.any(both[0] == CANARY) and len(np.unique(both[0])) > 1          # (written whole; the sphere is seen)
    for k in range(2):
        lone, _ = _call("sdfk_raymarch", pre, outs, _Scalars(), only=k)
        assert lone[k].tobytes() == both[k].tobytes() and lone[1 - k] is None, k
    _call("sdfk_raymarch", pre, outs, _Scalars(), only=-1)                         # (nothing asked for: not an error)
