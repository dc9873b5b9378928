"""The clouds of the filter stress tests (tests/test_points_filter_stress_cases.py on the CPU, tests/test_gpu_points_filter_stress.py
on the device) for KdTree.VoxelDownsample and KdTree.RemoveStatisticalOutliers: zero-spread clouds at every kind of accepted ratio,
clouds scaled until their float32 d2 are subnormal or overflow in part of a row, voxel populations on either side of the 32-member
chunk at segment starts that are no multiple of 32, and the split of a cloud for a tree grown with AddPoints.  Not a test module.
Every cloud is made from fixed seeds; tests/points_filter_model.py and tests/pointcloud_color_model.py are the yardsticks."""
import functools

import numpy as np

from tests import points_filter_model as FM

f32, f64 = np.float32, np.float64

# 0, the largest kind of finite ratio, and one that float32 does not hold exactly (the member takes a double and rounds it)
RATIOS = (0.0, 3e38, 0.1)
SCALES = (-70, 40, 70)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def recorded():
    """The recorded sphere with 20 strays of tests/test_points_filter_model.py."""
    from tests.test_points_filter_model import recorded_case
    return _frozen(recorded_case()[0])


# ---- zero spread: every mean distance equal, sigma == 0 ----
def duplicates():
    """40 copies of one point, k = 8: every mean is 0."""
    return _frozen(np.tile(np.array([[0.25, 0.5, 0.75]], f32), (40, 1))), 8


def unit_lattice():
    """A 6 x 6 x 6 unit lattice in random order, k = 2: every mean is 1."""
    g = np.arange(6, dtype=f32)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return _frozen(P[np.random.default_rng(81).permutation(len(P))].astype(f32)), 2


# ---- scale ----
@functools.lru_cache(maxsize=None)
def scaled(e, count=600):
    """The first `count` points of the recorded case times 2^e, exactly."""
    P = recorded()[:count]
    S = (P * f32(2.0 ** e)).astype(f32)
    assert np.array_equal(S.astype(f64), P.astype(f64) * 2.0 ** e)
    return _frozen(S)


VOXEL = 0.25          # the voxel of the scaled downsample, times 2^e; its origin, times 2^e
ORIGIN = (0.125, -0.5, 0.0625)


def scaled_lattice(e):
    """-> (voxel size, origin) of the scaled downsample as float32, exact."""
    s = f32(2.0 ** e)
    return f32(VOXEL) * s, tuple(f32(o) * s for o in ORIGIN)


# ---- chunk edges ----
POPULATIONS = (1, 32, 33, 31, 64, 65, 63, 96, 97)       # in voxel order along x: no segment but the first starts at a multiple of 32


CHUNK_ORIGIN = (0.0, -0.5, -0.5)    # y and z of every point lie in (-0.5, 0.5): one voxel of edge 1 that holds both signs


def cancelling(rs, count):
    """`count` float32 values in (-0.45, 0.45) whose sum nearly cancels: a third are random b, a third the same -b, the rest span
    2^-45 .. 2^-40.  The exact sum is that of the small ones, far below a unit in the last place of the binary64 partial sums, so
    the order of the additions shows in the float32 result, not just in the binary64 one."""
    big = (rs.random(count // 3) * 0.9 - 0.45).astype(f32)
    small = (rs.random(count - 2 * len(big)) * 2.0 ** rs.integers(-45, -39, count - 2 * len(big))).astype(f32)
    return rs.permutation(np.concatenate([big, -big, small]))


@functools.lru_cache(maxsize=None)
def chunk_edges():
    """-> (points, colours): voxel v along x holds POPULATIONS[v] points, in random insertion order (lattice: edge 1 at
    CHUNK_ORIGIN).  x - v spans 45 binary orders of magnitude (tests/points_filter_model.mixed_magnitudes); y, z and the three
    colour channels of every voxel cancel (cancelling), so that the order of the additions shows in the float32 outputs."""
    rs = np.random.default_rng(82)
    vox = np.repeat(np.arange(len(POPULATIONS)), POPULATIONS)
    n = len(vox)
    P = FM.mixed_magnitudes(rs, n, 0.999)
    P[:, 0] += vox.astype(f32)
    col = np.zeros((n, 3), f32)
    at = 0
    for count in POPULATIONS:
        for a in (1, 2):
            P[at:at + count, a] = cancelling(rs, count)
        for a in range(3):
            col[at:at + count, a] = f32(4) * cancelling(rs, count)
        at += count
    order = rs.permutation(n)
    return _frozen(P[order].astype(f32)), _frozen(col[order].astype(f32))


# ---- grown trees ----
@functools.lru_cache(maxsize=None)
def grown():
    """-> (points, a): a cloud of 3000 points for both filters -- clustered, so that voxels hold points from either side of the
    split -- and the number of points the tree is made from before AddPoints adds the rest; no multiple of 256."""
    rs = np.random.default_rng(83)
    P = (rs.integers(0, 12, (3000, 3)) * 0.5 + FM.mixed_magnitudes(rs, 3000, 0.499)).astype(f32)
    return _frozen(P), 1301
