"""CPU proof that the clouds of tests/points_filter_stress_cases.py have the properties the device tests
(tests/test_gpu_points_filter_stress.py) rely on, by the numpy models alone: zero spread keeps everything at every accepted ratio
and gives no NaN; at 2^70 the float32 d2 overflow for part of the rows only; at 2^-70 they are subnormal and their rounding shows;
the chunk-edge cloud has the populations and the unaligned segment starts it is there for; scaling a cloud and its lattice by a power
of two changes no group."""
import numpy as np
import pytest

from tests import pointcloud_color_model as CM
from tests import points_filter_model as FM
from tests import points_filter_stress_cases as SC
from tests import points_knn_model as KM
from tests.test_points_filter_model import bits, same, slow_downsample

f32, f64 = np.float32, np.float64


def test_the_ratios_are_accepted_and_one_is_inexact_in_float32():
    assert all(0 <= f32(r) < np.inf for r in SC.RATIOS) and f64(f32(0.1)) != 0.1 and f32(3e38) > 2.0 ** 127


@pytest.mark.parametrize("cloud", [SC.duplicates, SC.unit_lattice])
def test_zero_spread_keeps_everything_at_every_accepted_ratio(cloud):
    P, k = cloud()
    mean = FM.row_means(P, k)
    assert (mean == mean[0]).all()
    for ratio in SC.RATIOS:
        out = FM.outliers(P, k, ratio)
        assert list(out["stats"][:3]) == [len(P), 0, 0] and out["sigma"] == 0 and out["thr"] == out["mu"] == mean[0]
    with np.errstate(all="ignore"):                                       # what an infinite ratio would do: the reason it is refused
        assert np.isnan(FM.threshold(mean, np.inf)[2])
    with pytest.raises(FM.Refused):
        FM.outliers(P, k, np.inf)


def test_recorded_case_at_the_ratios():
    P = SC.recorded()
    kept = [int(FM.outliers(P, 8, r)["stats"][0]) for r in SC.RATIOS]
    assert 0 < kept[0] < kept[2] < kept[1] == len(P)                     # ratio 0: about half; 0.1: a few more; 3e38: everything


def test_at_2_70_d2_overflows_in_part_of_the_rows():
    S = SC.scaled(70)
    out = FM.outliers(S, 8, 1.0)
    kept, removed, isolated = (int(v) for v in out["stats"][:3])
    assert isolated == 574 and kept + removed == 26                      # only pairs closer than 2^-6 of the radius have a finite d2
    _, _, found = KM.knn(S, S, 8)
    assert found.min() == 1 and 1 < found.max() < 8                      # no row is full: part of every row overflowed
    assert not np.isnan(out["mean_distance"]).any() and np.isfinite([out["mu"], out["sigma"], out["thr"]]).all()


def test_at_2_40_the_statistics_are_the_unscaled_ones_rescaled():
    a, b = FM.outliers(SC.scaled(0), 8, 1.0), FM.outliers(SC.scaled(40), 8, 1.0)
    assert np.array_equal(a["keep"], b["keep"]) and b["mu"] == a["mu"] * 2.0 ** 40 and b["sigma"] == a["sigma"] * 2.0 ** 40


def test_at_2_minus_70_the_subnormal_roundings_show():
    a, b = FM.outliers(SC.scaled(-60), 8, 1.0), FM.outliers(SC.scaled(-70), 8, 1.0)
    assert b["stats"][2] == 0 and 0 < b["mu"] < 2.0 ** -70 and b["mu"] != a["mu"] * 2.0 ** -10
    _, d, _ = KM.knn(SC.scaled(-70), SC.scaled(-70)[:100], 8)
    assert (d.astype(f64) ** 2).max() < 2.0 ** -126                        # every d2 of a row is subnormal
    assert not np.isnan(b["mean_distance"]).any()


def _chain_mean(values):
    """The mean by one sequential binary64 chain in ascending index: what a sum without the chunks would give."""
    total = np.zeros(values.shape[1], f64)
    for v in values:
        total = total + v.astype(f64)
    return (total / f64(len(values))).astype(f32)


def test_chunk_edge_cloud_has_the_populations_at_unaligned_starts():
    P, col = SC.chunk_edges()
    pts, cnt, group = FM.voxel_downsample(P, 1.0, SC.CHUNK_ORIGIN)
    assert sorted(cnt) == sorted(SC.POPULATIONS) and set(SC.POPULATIONS) >= {1, 31, 32, 33, 63, 64, 65, 96, 97}
    keys, _ = FM.voxel_keys(P, 1.0, SC.CHUNK_ORIGIN)
    by_key = np.bincount(keys.astype(np.int64))
    assert tuple(by_key) == SC.POPULATIONS
    starts = np.cumsum(by_key)[:-1]                                       # the sorted positions the segments after the first begin at
    assert (starts % 32 != 0).all()
    assert same((pts, cnt, group), slow_downsample(P, 1.0, SC.CHUNK_ORIGIN))
    cpts, ccnt, cgroup, ccol = CM.voxel_downsample(P, col, 1.0, SC.CHUNK_ORIGIN)
    assert same((cpts, ccnt, cgroup), (pts, cnt, group)) and ccol.shape == pts.shape and not np.isnan(ccol).any()
    # the order of the additions shows in the float32 outputs: a plain chain gives other centroids and other colours in every voxel
    # whose second chunk holds more than one member (one chunk IS a chain, and so is a chunk and a single member: 0.0 + x = x)
    for g in range(len(cnt)):
        members = np.nonzero(group == g)[0]
        chain_p, chain_c = _chain_mean(P[members]), _chain_mean(col[members])
        if cnt[g] <= 33:
            assert np.array_equal(bits(chain_p), bits(pts[g])) and np.array_equal(bits(chain_c), bits(ccol[g]))
        else:
            assert (bits(chain_p) != bits(pts[g])).any() and (bits(chain_c) != bits(ccol[g])).any(), cnt[g]


@pytest.mark.parametrize("e", SC.SCALES)
def test_scaling_cloud_and_lattice_changes_no_group(e):
    size, origin = SC.scaled_lattice(e)
    base = FM.voxel_downsample(SC.scaled(0), *SC.scaled_lattice(0))
    got = FM.voxel_downsample(SC.scaled(e), size, origin)
    assert np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2]) and 100 < len(got[0]) < 600 and got[1].max() >= 3
    assert np.array_equal(got[0].astype(f64), base[0].astype(f64) * 2.0 ** e) and np.isfinite(got[0]).all()


def test_grown_cloud_splits_off_a_block_edge_and_mixes_the_halves():
    P, a = SC.grown()
    assert a % 256 != 0 and 0 < a < len(P)
    _, cnt, group = FM.voxel_downsample(P, 0.5)
    mixed = np.intersect1d(group[:a], group[a:])
    assert len(mixed) > 100 and cnt.max() > 2                             # voxels with members on both sides of the split
    out = FM.outliers(P, 8, 1.0)
    assert out["stats"][1] > 0 and out["keep"][:a].any() and out["keep"][a:].any() and not out["keep"].all()
