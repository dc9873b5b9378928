"""A numpy restatement of the KdTree's two filters (include/sdfkit_hip.h, "Point clouds: filters"), the yardstick of
sdfkit_amd.points.KdTree.VoxelDownsample / RemoveStatisticalOutliers (csrc/lib_points_filter.hip, csrc/points_filter.h).  Not a
test module.  One numpy float64 operation per written operation of the contract (numpy has no FMA).

- voxel_downsample(): keys from floor((p - o) / size) in float64; groups by np.lexsort / np.unique (members in ascending index,
  voxels in the order of their lowest member); the centroid sums in chunks of 32 -- 32 vectorised steps over all chunks at once,
  then one step per chunk rank over all voxels at once.
- outliers(): the k-nearest rows of tests/points_knn_model.py; the statistics in the reduction order of sdfk_icp_register's step 1,
  which tests/points_model.py states (reduce_fixed).
"""
import numpy as np

from tests import points_knn_model as KM
from tests import points_model as PM

f32, f64 = np.float32, np.float64
CHUNK = 32
AXIS_SPAN = 1 << 21


def mixed_magnitudes(rs, n, top=1.0):
    """(n, 3) float32 in [0, top) whose magnitudes span 2^-45 .. 1: binary64 sums of such values are inexact, so the order of the
    additions shows in the result (f32 values of like magnitude sum exactly in binary64, in any order)."""
    return (rs.random((n, 3)) * top * 2.0 ** rs.integers(-45, 1, (n, 3))).astype(f32)


class Refused(ValueError):
    """What the library answers with SDFK_ERR_INVALID."""


def voxel_of(p, o, size):
    """floor(((double)p - (double)o) / (double)size): integer-valued float64."""
    with np.errstate(all="ignore"):
        return np.floor((np.asarray(p, f32).astype(f64) - f64(f32(o))) / f64(f32(size)))


def voxel_keys(P, size, origin=(0, 0, 0)):
    """-> (packed keys uint64 (n,), kmin (3,) float64); raises Refused as the library refuses."""
    P = np.ascontiguousarray(np.asarray(P, f32).reshape(-1, 3))
    size = f32(size)
    o = np.asarray(origin, f32).reshape(3)
    if not (np.isfinite(size) and size > 0):
        raise Refused("size")
    if not np.isfinite(o).all():
        raise Refused("origin")
    k = np.stack([voxel_of(P[:, a], o[a], size) for a in range(3)], axis=1)
    kmin, kmax = k.min(axis=0), k.max(axis=0)
    with np.errstate(all="ignore"):
        if not ((kmax - kmin) < f64(AXIS_SPAN)).all():
            raise Refused("span")
    d = (k - kmin).astype(np.uint64)
    return d[:, 2] << np.uint64(42) | d[:, 1] << np.uint64(21) | d[:, 0], kmin


def passes(P, size, origin=(0, 0, 0)):
    """The 8-bit digits of the packed key the three ranges can set, as the sort takes them: a list of digit numbers."""
    P = np.ascontiguousarray(np.asarray(P, f32).reshape(-1, 3))
    o = np.asarray(origin, f32).reshape(3)
    out = set()
    for a in range(3):
        k = voxel_of(P[:, a], o[a], size)
        bits = int(k.max() - k.min()).bit_length()
        out |= {b >> 3 for b in range(21 * a, 21 * a + bits)}
    return sorted(out)


def chunked_sums(values, seg, rank, m):
    """values (n, K) float64, already in (voxel, ascending index) order; seg (n,) the voxel of each row, rank (n,) its rank within the
    voxel -> (m, K): per voxel the chunk sums (each summed in order from +0.0) added in order to +0.0."""
    values = np.asarray(values, f64)
    n, K = values.shape
    chunk = rank // CHUNK
    # a number for every chunk: chunks of a voxel are consecutive
    first_row = np.flatnonzero(rank == 0)
    counts = np.diff(np.append(first_row, n))
    nchunks = (counts + CHUNK - 1) // CHUNK
    chunk_base = np.concatenate([[0], np.cumsum(nchunks)])
    cid = chunk_base[seg] + chunk
    csum = np.zeros((int(chunk_base[-1]), K), f64)
    within = rank % CHUNK
    for t in range(CHUNK):                       # 32 vectorised steps over all chunks
        rows = np.flatnonzero(within == t)
        if not len(rows):
            break
        csum[cid[rows]] = csum[cid[rows]] + values[rows]
    total = np.zeros((m, K), f64)
    for q in range(int(nchunks.max()) if m else 0):    # one step per chunk rank
        vox = np.flatnonzero(nchunks > q)
        total[vox] = total[vox] + csum[chunk_base[vox] + q]
    return total, counts


def voxel_downsample(P, size, origin=(0, 0, 0)):
    """-> (points (m, 3) float32, counts (m,) int32, group (n,) int32)."""
    P = np.ascontiguousarray(np.asarray(P, f32).reshape(-1, 3))
    n = len(P)
    keys, _ = voxel_keys(P, size, origin)
    order = np.lexsort((np.arange(n), keys))                      # by key, members in ascending index
    uniq, first, inverse = np.unique(keys, return_index=True, return_inverse=True)   # first: the lowest member of each voxel
    m = len(uniq)
    out_of_key = np.empty(m, np.int64)
    out_of_key[np.argsort(first, kind="stable")] = np.arange(m)  # voxels in the order of their lowest member
    group = out_of_key[inverse]
    seg_sorted = inverse[order]                                   # the voxel (in key order) of each sorted row
    start = np.flatnonzero(np.concatenate([[True], seg_sorted[1:] != seg_sorted[:-1]]))
    rank = np.arange(n) - start[seg_sorted]
    total, counts = chunked_sums(P[order].astype(f64), seg_sorted, rank, m)
    with np.errstate(all="ignore"):
        cent = (total / counts[:, None].astype(f64)).astype(f32)
    pts = np.empty((m, 3), f32)
    cnt = np.empty(m, np.int32)
    pts[out_of_key] = cent
    cnt[out_of_key] = counts
    return pts, cnt, group.astype(np.int32)


def row_means(P, k, max_distance=np.inf, knn=None):
    """mean_i (float64; +inf: isolated) of every point.  knn: the (distance (n, k) float32, found (n,)) of the rows, when the caller
    has them from a cheaper exact route than the brute force of tests/points_knn_model.py."""
    P = np.ascontiguousarray(np.asarray(P, f32).reshape(-1, 3))
    dist, found = knn if knn is not None else KM.knn(P, P, k, max_distance)[1:]
    n = len(P)
    s = np.zeros(n, f64)
    with np.errstate(all="ignore"):
        for j in range(1, int(k)):                                # in row order, from 0.0; the first entry is dropped
            live = found > j
            s = np.where(live, s + dist[:, j].astype(f64), s)
        mean = np.where(found >= 2, s / np.maximum(found - 1, 1).astype(f64), np.inf)
    return mean


def threshold(mean, std_ratio):
    """-> (mu, sigma, thr, c) from the means (+inf: takes no part)."""
    part = mean < np.inf
    c = int(part.sum())
    if c == 0:
        return f64(0.0), f64(0.0), f64(0.0), 0
    with np.errstate(all="ignore"):
        mu = PM.reduce_fixed(np.where(part, mean, 0.0)) / f64(c)
        d = np.where(part, mean, mu) - mu
        sigma = np.sqrt(PM.reduce_fixed(np.where(part, d * d, 0.0)) / f64(c))
        thr = mu + f64(f32(std_ratio)) * sigma
    return mu, sigma, thr, c


def outliers(P, k, std_ratio, max_distance=np.inf, knn=None):
    """-> dict: mean_distance (n,) float32, keep (n,) uint8, index (kept,) int32, points (kept, 3) float32, stats (6 int64)."""
    P = np.ascontiguousarray(np.asarray(P, f32).reshape(-1, 3))
    k = int(k)
    if not 2 <= k <= 64:
        raise Refused("k")
    with np.errstate(over="ignore"):                              # (a double beyond FLT_MAX is +inf as the float argument)
        if not 0 <= f32(std_ratio) < np.inf:                      # finite and not negative (NaN fails both)
            raise Refused("std_ratio")
    if not f32(max_distance) >= 0:
        raise Refused("max_distance")
    mean = row_means(P, k, max_distance, knn)
    mu, sigma, thr, c = threshold(mean, std_ratio)
    keep = (mean < np.inf) & (mean <= thr)
    idx = np.flatnonzero(keep).astype(np.int32)
    kept = len(idx)
    bits = np.array([mu, sigma, thr], f64).view(np.int64)
    with np.errstate(all="ignore"):
        md = mean.astype(f32)
    return {"mean_distance": md, "keep": keep.astype(np.uint8), "index": idx, "points": P[idx],
            "stats": np.array([kept, c - kept, len(P) - c, bits[0], bits[1], bits[2]], np.int64), "mu": mu, "sigma": sigma, "thr": thr}
