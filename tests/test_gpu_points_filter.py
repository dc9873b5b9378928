"""KdTree.VoxelDownsample and KdTree.RemoveStatisticalOutliers on the MI355X (csrc/lib_points_filter.hip) against the numpy model
(tests/points_filter_model.py), bit for bit: every output array, m, n_kept and all six stats, in the host and the device form; the
shapes are the smallest at which the radix sort (tiles of TILE records, one to several digit passes), the segment sums and the
second stride of the reduction can go wrong.  Then two tests of what the filters are for."""
import ctypes as C

import numpy as np
import pytest

from sdfkit_amd import _native as N
from sdfkit_amd.points import KdTree
from tests import points_filter_model as FM
from tests.test_points_filter_model import bits, recorded_case

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TILE = 2048   # kSortTile of csrc/lib_points_filter.hip: keep them equal
INF = np.inf


# ---- downsample ----
def lattice_cloud(seed, n, dims):
    """n points in a lattice of dims = (nx, ny, nz) unit voxels, in random order: the x and z offsets within a voxel span 45 binary
    orders of magnitude where the voxel number is 0, so that the order of a voxel's additions shows in its centroid."""
    rs = np.random.default_rng(seed)
    vox = np.stack([rs.integers(0, d, n) for d in dims], axis=1)
    return (vox + FM.mixed_magnitudes(rs, n, 0.999)).astype(f32)


def downsample_device(tree, size, origin=(0, 0, 0)):
    import torch
    n = tree.TotalPoints
    N.bind_torch_stream()
    dev = torch.device("cuda:0")
    pts = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    grp = torch.full((n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    o = (C.c_float * 3)(*[float(v) for v in origin])
    m = C.c_int64(-1)
    N.check(N.lib().sdfk_points_voxel_downsample_device(tree.handle, float(f32(size)), o, C.c_void_p(pts.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                         C.c_void_p(grp.data_ptr()), C.byref(m)))
    # (the call has finished when it returns)
    pts, cnt, grp = pts.cpu().numpy(), cnt.cpu().numpy(), grp.cpu().numpy()
    assert (pts[m.value:] == -7).all() and (cnt[m.value:] == -7).all()      # entries from m on are left alone
    return pts[:m.value], cnt[:m.value], grp


def check_downsample(P, size, origin=(0, 0, 0), device=True, tree=None):
    """tree: a tree that holds P already (one grown with AddPoints, for one); else one is made from P."""
    want = FM.voxel_downsample(P, size, origin)
    tree = tree or KdTree(P)
    assert tree.TotalPoints == len(P)
    forms = [tree.VoxelDownsample(size, origin)] + ([downsample_device(tree, size, origin)] if device else [])
    for got in forms:
        assert len(got[0]) == len(want[0])                                   # m
        assert np.array_equal(got[2], want[2])                              # group
        assert np.array_equal(got[1], want[1])                              # counts
        assert np.array_equal(bits(got[0]), bits(want[0]))                  # points_out
    return want


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, 3 * TILE + 17])
def test_downsample_around_the_tile_size(gpu, n):
    P = lattice_cloud(n, n, (7, 5, 3))
    want = check_downsample(P, 1.0)
    assert FM.passes(P, 1.0) == ([0, 2, 5] if n > 1 else []) and len(want[0]) == min(n, 105)


def test_downsample_200000_points(gpu):
    P = lattice_cloud(1, 200_000, (40, 30, 20))
    want = check_downsample(P, 1.0)
    assert 23_900 < len(want[0]) <= 24_000 and want[1].max() > 16


def test_downsample_one_digit_pass(gpu):
    P = lattice_cloud(2, 3 * TILE + 17, (200, 1, 1))
    assert FM.passes(P, 1.0) == [0]
    assert len(check_downsample(P, 1.0)[0]) == 200


def test_downsample_many_digit_passes(gpu):
    """2^18 voxels and more: 9 bits of x (digits 0, 1), 6 of y (2, 3), 6 of z (5)."""
    P = lattice_cloud(3, 20_000, (300, 64, 64))
    assert FM.passes(P, 1.0) == [0, 1, 2, 3, 5]
    want = check_downsample(P, 1.0)
    assert len(want[0]) > 19_000
    # ... and all 8 digits: 21 bits along every axis
    Q = (lattice_cloud(4, 5000, (3, 3, 3)) * f32(1000)).astype(f32)
    assert FM.passes(Q, 0.0015) == list(range(8))
    check_downsample(Q, 0.0015)


def test_downsample_heavy_duplication(gpu):
    P = lattice_cloud(5, 100_000, (1, 50, 1))
    want = check_downsample(P, 1.0)
    assert len(want[0]) == 50 and want[1].min() > 1500


def test_downsample_all_in_one_voxel(gpu):
    P = lattice_cloud(6, 1000, (1, 1, 1))
    want = check_downsample(P, 1.0)
    assert len(want[0]) == 1 and want[1][0] == 1000 and FM.passes(P, 1.0) == []
    chain = np.zeros(3, f64)
    for p in P:
        chain = chain + p.astype(f64)
    total, _ = FM.chunked_sums(P.astype(f64), np.zeros(1000, np.int64), np.arange(1000), 1)
    assert not np.array_equal(chain, total[0])      # (the case tells the chunked order from a chain)


def test_downsample_identity_below_the_spacing(gpu):
    rs = np.random.default_rng(7)
    P = (rs.permutation(20_000)[:5000, None] * f32(0.01) + rs.random((5000, 3)) * 0.001 + 0.01).astype(f32)
    pts, cnt, group = check_downsample(P, 0.002, (0.0005, 0, -1))
    assert np.array_equal(bits(pts), bits(P)) and (cnt == 1).all() and np.array_equal(group, np.arange(5000))


def test_downsample_merged_sphere(gpu):
    P = recorded_case()[0][:2000]
    M = np.concatenate([P, (P + f32(0.001)).astype(f32)])
    pts, cnt, group = check_downsample(M, 0.1)
    assert len(pts) == 1079 and cnt.max() == 16


def test_downsample_negative_coordinates_and_origin(gpu):
    rs = np.random.default_rng(8)
    P = (rs.standard_normal((3 * TILE, 3)) * 3).astype(f32)
    P[:50] = rs.integers(-4, 5, (50, 3)) * f32(0.5)             # on voxel faces, both signs of zero
    P[50:60] *= f32(-0.0)
    check_downsample(P, 0.5)
    check_downsample(P, 0.37, (0.1, -7.5, 3.25))


def test_downsample_refusals(gpu):
    tree = KdTree(np.array([[0, 0, 0], [2 ** 21, 1, 1]], f32))
    for size, origin in ((1.0, (0, 0, 0)), (0.0, (0, 0, 0)), (-1.0, (0, 0, 0)), (INF, (0, 0, 0)), (np.nan, (0, 0, 0)), (2.0, (np.nan, 0, 0))):
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.VoxelDownsample(size, origin)
        assert e.value.status == N.ERR_INVALID
    assert len(tree.VoxelDownsample(1.0001)[0]) == 2            # 2^21 - 1 voxels apart: accepted


# ---- outliers ----
def outliers_device(tree, k, ratio, maxd):
    import torch
    n = tree.TotalPoints
    N.bind_torch_stream()
    dev = torch.device("cuda:0")
    mean = torch.empty((n,), dtype=torch.float32, device=dev)
    keep = torch.empty((n,), dtype=torch.uint8, device=dev)
    idx = torch.full((n,), -7, dtype=torch.int32, device=dev)
    pts = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    kept = C.c_int64(-1)
    st = (C.c_int64 * 6)()
    N.check(N.lib().sdfk_points_outliers_device(tree.handle, int(k), float(f32(ratio)), float(f32(maxd)), C.c_void_p(mean.data_ptr()),
                                                C.c_void_p(keep.data_ptr()), C.c_void_p(idx.data_ptr()), C.c_void_p(pts.data_ptr()), C.byref(kept), st))
    idx, pts = idx.cpu().numpy(), pts.cpu().numpy()
    assert (idx[kept.value:] == -7).all() and (pts[kept.value:] == -7).all()
    return {"mean_distance": mean.cpu().numpy(), "keep": keep.cpu().numpy(), "index": idx[:kept.value], "points": pts[:kept.value],
            "stats": np.array(list(st), np.int64)}


def outliers_host(tree, k, ratio, maxd):
    n = tree.TotalPoints
    mean, keep = np.empty(n, f32), np.empty(n, np.uint8)
    idx, pts = np.empty(n, np.int32), np.empty((n, 3), f32)
    kept = C.c_int64(-1)
    st = (C.c_int64 * 6)()
    p = lambda a: C.c_void_p(a.ctypes.data)
    N.check(N.lib().sdfk_points_outliers(tree.handle, int(k), float(f32(ratio)), float(f32(maxd)), p(mean), p(keep), p(idx), p(pts), C.byref(kept), st))
    return {"mean_distance": mean, "keep": keep, "index": idx[:kept.value], "points": pts[:kept.value], "stats": np.array(list(st), np.int64)}


def check_outliers(P, k, ratio, maxd=INF, knn=None, tree=None):
    """tree: a tree that holds P already; else one is made from P."""
    want = FM.outliers(P, k, ratio, maxd, knn)
    tree = tree or KdTree(P)
    assert tree.TotalPoints == len(P)
    for got in (outliers_host(tree, k, ratio, maxd), outliers_device(tree, k, ratio, maxd)):
        assert np.array_equal(bits(got["mean_distance"]), bits(want["mean_distance"]))
        assert np.array_equal(got["stats"], want["stats"]), (got["stats"], want["stats"])
        assert np.array_equal(got["keep"], want["keep"])
        assert np.array_equal(got["index"], want["index"])
        assert np.array_equal(bits(got["points"]), bits(want["points"]))
    # the Python member returns the same
    stats = {}
    pts, idx, mean = tree.RemoveStatisticalOutliers(k, ratio, maxd, stats)
    assert np.array_equal(bits(pts), bits(want["points"])) and np.array_equal(idx, want["index"]) and np.array_equal(bits(mean), bits(want["mean_distance"]))
    assert [stats["kept"], stats["removed"], stats["isolated"]] == list(want["stats"][:3])
    assert np.array_equal(np.array([stats["mu"], stats["sigma"], stats["threshold"]], f64).view(np.int64), want["stats"][3:])
    return want


@pytest.mark.parametrize("k", [2, 8, 16, 32, 64])
def test_outliers_recorded_case_in_every_tier(gpu, k):
    P, strays = recorded_case()
    want = check_outliers(P, k, 2.0)
    assert want["stats"][2] == 0 and not want["keep"][strays].any()
    if k in (8, 16):
        assert list(want["stats"][:3]) == [2000, 20, 0]


def line_cloud(n, k, seed=11, window=24):
    """n points along x in ascending order with gaps of uneven size, and their exact k-nearest rows from the `window` points on
    either side (every other point is farther than the k-th found: asserted)."""
    rs = np.random.default_rng(seed)
    gaps = f64(1e-3) * (1.0 + 3.0 * rs.random(n) ** 4)
    P = np.stack([np.cumsum(gaps), rs.random(n) * 3e-4, rs.random(n) * 3e-4], axis=1).astype(f32)
    j = np.arange(n)[:, None] + np.arange(-window, window + 1)[None, :]
    ok = (j >= 0) & (j < n)
    Q = P[np.clip(j, 0, n - 1)]
    d = P[:, None, :] - Q
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d2 = np.where(ok, d2, f32(np.inf)).astype(f32)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]            # (candidates ascend in index: stable = ties to the lower index)
    dist = np.sqrt(np.take_along_axis(d2, order, axis=1).astype(f64)).astype(f32)
    x = P[:, 0].astype(f64)
    beyond = np.minimum(np.where(np.arange(n) + window + 1 < n, np.roll(x, -(window + 1)) - x, np.inf),
                        np.where(np.arange(n) - window - 1 >= 0, x - np.roll(x, window + 1), np.inf))
    assert (dist[:, -1].astype(f64) * 1.001 < beyond).all()
    return P, (dist, np.full(n, k, np.int32))


def test_outliers_70000_points_reach_the_second_stride(gpu):
    P, knn = line_cloud(70_000, 8)
    want = check_outliers(P, 8, 1.0, knn=knn)
    assert want["stats"][1] > 100 and want["stats"][0] > 50_000
    assert want["keep"][65_536:].any() and not want["keep"][65_536:].all()


def test_outliers_duplicates(gpu):
    rs = np.random.default_rng(12)
    P = rs.random((1500, 3)).astype(f32)
    P[500:800] = P[:300]                     # pairs
    P[800:900] = P[0]                        # a point held 102 times: at k = 8 its rows are all zeros
    want = check_outliers(P, 8, 1.5)
    assert (want["mean_distance"][800:900] == 0).all() and want["stats"][1] > 0


def test_outliers_finite_max_distance_isolates_some(gpu):
    P, strays = recorded_case()
    want = check_outliers(P, 8, 2.0, 0.05)
    assert 0 < want["stats"][2] < len(P) and np.isinf(want["mean_distance"][strays]).all() and want["stats"][0] > 0


def test_outliers_everything_isolated(gpu):
    P, _ = recorded_case()
    want = check_outliers(P[:300], 4, 1.0, 1e-6)
    assert list(want["stats"]) == [0, 0, 300, 0, 0, 0] and len(want["index"]) == 0


def test_outliers_refusals(gpu):
    tree = KdTree(recorded_case()[0][:100])
    for k, ratio, maxd in ((1, 1.0, INF), (65, 1.0, INF), (8, -0.5, INF), (8, np.nan, INF), (8, 1.0, -1.0), (8, 1.0, np.nan)):
        with pytest.raises(N.SdfKitNativeError) as e:
            tree.RemoveStatisticalOutliers(k, ratio, maxd)
        assert e.value.status == N.ERR_INVALID
    # an infinite ratio: inf * sigma is a NaN where sigma == 0.  Refused by both entry points and the member, everything left as it was
    import torch
    n = tree.TotalPoints
    with pytest.raises(N.SdfKitNativeError) as e:
        tree.RemoveStatisticalOutliers(8, INF)
    assert e.value.status == N.ERR_INVALID
    mean, keep = np.full(n, -7, f32), np.full(n, 7, np.uint8)
    idx, pts = np.full(n, -7, np.int32), np.full((n, 3), -7, f32)
    kept = C.c_int64(-7)
    st = (C.c_int64 * 6)(*[-7] * 6)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert N.lib().sdfk_points_outliers(tree.handle, 8, float(INF), float(INF), p(mean), p(keep), p(idx), p(pts), C.byref(kept), st) == N.ERR_INVALID
    assert (mean == -7).all() and (keep == 7).all() and (idx == -7).all() and (pts == -7).all() and kept.value == -7 and list(st) == [-7] * 6
    N.bind_torch_stream()
    try:
        dev = torch.device("cuda:0")
        dm, dk = torch.full((n,), -7.0, dtype=torch.float32, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev)
        di, dp = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        d = lambda t: C.c_void_p(t.data_ptr())
        assert N.lib().sdfk_points_outliers_device(tree.handle, 8, float(INF), float(INF), d(dm), d(dk), d(di), d(dp), C.byref(kept), st) == N.ERR_INVALID
        N.check(N.lib().sdfk_synchronize())
        torch.cuda.synchronize()
        assert (dm == -7).all() and (dk == 7).all() and (di == -7).all() and (dp == -7).all() and kept.value == -7 and list(st) == [-7] * 6
    finally:
        N.check(N.lib().sdfk_set_stream(None))
    assert tree.RemoveStatisticalOutliers(8, 3e38)[1].tolist() == list(range(n))      # the largest ratios are accepted: nothing goes


# ---- what the filters are for ----
def test_centroids_lie_in_their_voxels_and_a_second_pass_changes_nothing(gpu):
    rs = np.random.default_rng(13)
    P = (rs.standard_normal((30_000, 3)) * 2 + 0.3).astype(f32)
    size, origin = f32(0.25), np.array([0.1, 0.2, -0.3], f32)
    tree = KdTree(P)
    pts, cnt, group = tree.VoxelDownsample(size, origin)
    assert cnt.sum() == len(P) and len(pts) < len(P) and cnt.max() >= 4
    vox = np.floor((P.astype(f64) - origin.astype(f64)) / f64(size))
    centre = (vox[np.unique(group, return_index=True)[1]] + 0.5) * f64(size) + origin.astype(f64)   # (group numbers ascend with the lowest member)
    assert (np.abs(pts.astype(f64) - centre) <= f64(size) / 2 * (1 + 1e-6)).all()
    again = KdTree(pts).VoxelDownsample(size, origin)
    assert np.array_equal(bits(again[0]), bits(pts)) and (again[1] == 1).all() and np.array_equal(again[2], np.arange(len(pts)))


def test_removing_the_stray_point_gives_the_grid_back(gpu):
    """DESIGN.md section 8's weak case: one far point stretches the box and leaves the cloud in a few cells of the search grid."""
    rs = np.random.default_rng(14)
    P = np.concatenate([rs.random((10_000, 3)), [[1e6, 1e6, 1e6]]]).astype(f32)
    tree = KdTree(P)
    before = tree.stats()["grid"]
    cells_over_the_cube = np.prod([min(d, int(np.ceil(d / 1e6)) + 1) for d in before])     # (cell edge = 1e6 / d: the unit cube spans 1 or 2 cells)
    assert cells_over_the_cube <= 8
    pts, idx, _ = tree.RemoveStatisticalOutliers(8, 2.0)
    assert np.array_equal(idx, np.arange(10_000)) and np.array_equal(bits(pts), bits(P[:10_000]))
    after = KdTree(pts).stats()["grid"]
    assert int(np.prod(after)) >= 1000
