"""KdTree.VoxelDownsample (with and without colours) and KdTree.RemoveStatisticalOutliers on the MI355X on the clouds of
tests/points_filter_stress_cases.py against the numpy models (tests/points_filter_model.py, tests/pointcloud_color_model.py), bit for
bit in the host and the device form: zero-spread clouds at every kind of accepted ratio, float32 d2 that are subnormal or overflow in
part of a row, voxel populations on either side of the 32-member chunk at unaligned segment starts, trees grown with AddPoints.
What the clouds are there for is proved on the CPU in tests/test_points_filter_stress_cases.py; no compared value is a NaN."""
import ctypes as C

import numpy as np
import pytest

from sdfkit_amd import _native as N
from sdfkit_amd.points import KdTree
from tests import pointcloud_color_model as CM
from tests import points_filter_stress_cases as SC
from tests.test_gpu_points_filter import check_downsample, check_outliers
from tests.test_points_filter_model import bits

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def _no_nan(want):
    assert not np.isnan(want["mean_distance"]).any() and not np.isnan(want["stats"][3:].view(f64)).any()


# ---- outliers ----
@pytest.mark.parametrize("ratio", SC.RATIOS)
def test_outliers_recorded_case_at_the_edges_of_the_ratio(gpu, ratio):
    P = SC.recorded()
    want = check_outliers(P, 8, ratio)
    _no_nan(want)
    assert 0 < want["stats"][0] <= len(P) and (want["stats"][0] == len(P)) == (ratio == 3e38)


@pytest.mark.parametrize("ratio", SC.RATIOS)
@pytest.mark.parametrize("cloud", [SC.duplicates, SC.unit_lattice])
def test_outliers_zero_spread_keeps_everything(gpu, cloud, ratio):
    P, k = cloud()
    want = check_outliers(P, k, ratio)
    _no_nan(want)
    assert list(want["stats"][:3]) == [len(P), 0, 0] and want["sigma"] == 0 and want["keep"].all()


@pytest.mark.parametrize("e", SC.SCALES)
def test_outliers_at_scale(gpu, e):
    want = check_outliers(SC.scaled(e), 8, 1.0)
    _no_nan(want)
    if e == 70:                                   # d2 overflows for all but the closest pairs
        assert want["stats"][2] == 574 and want["stats"][0] + want["stats"][1] == 26 and np.isinf(want["mean_distance"]).sum() == 574
    else:
        assert want["stats"][2] == 0 and want["stats"][1] > 0


# ---- downsample ----
def _colours_device(tree, size, origin, col):
    import torch
    n = tree.TotalPoints
    N.bind_torch_stream()
    dev = torch.device("cuda:0")
    cd = torch.from_numpy(np.array(col, f32)).to(dev)
    pts, out = (torch.full((n, 3), -7.0, dtype=torch.float32, device=dev) for _ in range(2))
    cnt, grp = (torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    o = (C.c_float * 3)(*[float(v) for v in origin])
    m = C.c_int64(-1)
    p = lambda t: C.c_void_p(t.data_ptr())
    N.check(N.lib().sdfk_points_voxel_downsample_colors_device(tree.handle, float(f32(size)), o, p(cd), p(pts), p(cnt), p(grp), p(out), C.byref(m)))
    pts, cnt, grp, out = (t.cpu().numpy() for t in (pts, cnt, grp, out))           # (the call has finished when it returns)
    assert (pts[m.value:] == -7).all() and (cnt[m.value:] == -7).all() and (out[m.value:] == -7).all()
    return pts[:m.value], cnt[:m.value], grp, out[:m.value]


def test_downsample_chunk_edges_at_unaligned_segment_starts(gpu):
    P, col = SC.chunk_edges()
    tree = KdTree(P)
    want = check_downsample(P, 1.0, SC.CHUNK_ORIGIN, tree=tree)
    assert sorted(want[1]) == sorted(SC.POPULATIONS)
    wcol = CM.voxel_downsample(P, col, 1.0, SC.CHUNK_ORIGIN)
    for got in (tree.VoxelDownsample(1.0, SC.CHUNK_ORIGIN, colors=col), _colours_device(tree, 1.0, SC.CHUNK_ORIGIN, col)):
        assert len(got[0]) == len(wcol[0]) and np.array_equal(got[1], wcol[1]) and np.array_equal(got[2], wcol[2])
        assert np.array_equal(bits(got[0]), bits(wcol[0])) and np.array_equal(bits(got[3]), bits(wcol[3]))


@pytest.mark.parametrize("e", SC.SCALES)
def test_downsample_at_scale(gpu, e):
    size, origin = SC.scaled_lattice(e)
    want = check_downsample(SC.scaled(e), size, origin)
    assert 100 < len(want[0]) < 600 and np.isfinite(want[0]).all()


# ---- trees grown with AddPoints ----
def test_filters_on_a_grown_tree(gpu):
    P, a = SC.grown()
    tree = KdTree(P[:a])
    tree.AddPoints(P[a:])
    want = check_downsample(P, 0.5, tree=tree)
    assert want[1].max() > 2
    check_downsample(P, 0.37, (0.1, -7.5, 3.25), tree=tree)
    want = check_outliers(P, 8, 1.0, tree=tree)
    _no_nan(want)
    assert want["stats"][1] > 0
    check_outliers(P, 33, 0.5, 1.5, tree=tree)
