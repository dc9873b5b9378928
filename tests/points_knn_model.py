"""A numpy brute-force model of KdTree's k-nearest and radius queries (include/sdfkit_hip.h, "k nearest / within a radius"),
the yardstick of sdfkit_amd.points.KdTree.SearchKNearest / SearchRadius (csrc/lib_points_knn.hip).  Not a test module.

The contract's formula, as tests/points_model.nearest states it for one neighbour: d2 = (dx*dx + dy*dy) + dz*dz in float32
(numpy float32 arithmetic has no FMA); a point counts only if d2 < +inf; static points are ordered by (d2, index) -- a STABLE
sort of d2 resolves ties to the lower index; distance = sqrtf(d2) correctly rounded (float64 sqrt rounded to float32); a
counting point is within r iff that float32 distance is <= r.
"""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def _d2(P, q):
    with np.errstate(all="ignore"):
        dx = q[:, None, 0] - P[None, :, 0]
        dy = q[:, None, 1] - P[None, :, 1]
        dz = q[:, None, 2] - P[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    d2[~(d2 < np.inf)] = np.inf            # NaN / inf: does not count
    return d2


def _dist(d2):
    return np.sqrt(d2.astype(np.float64)).astype(f32)


def _arrays(static, queries):
    P = np.ascontiguousarray(np.asarray(static, f32).reshape(-1, 3))
    Q = np.ascontiguousarray(np.asarray(queries, f32).reshape(-1, 3))
    return P, Q


def _rows(d2, mask):
    """Per row: the indices where mask holds, ordered by (d2, index) -- nonzero yields ascending indices and the sort is stable."""
    for row, mrow in zip(d2, mask):
        j = np.nonzero(mrow)[0]
        yield j[np.argsort(row[j], kind="stable")]


def knn(static, queries, k, max_distance=np.inf, chunk_elems=1 << 23):
    """-> (index (m, k) int32, distance (m, k) float32, found (m,) int32); unused slots: -1 and FLT_MAX."""
    P, Q = _arrays(static, queries)
    m, k = len(Q), int(k)
    r = f32(max_distance)
    assert 1 <= k <= 64 and r >= 0
    idx = np.full((m, k), -1, np.int32)
    dist = np.full((m, k), FLT_MAX, f32)
    found = np.zeros(m, np.int32)
    step = max(1, chunk_elems // max(1, len(P)))
    kk = min(k, len(P))
    for a in range(0, m, step):
        d2 = _d2(P, Q[a:a + step])
        # every point up to the kk-th least d2 (ties of it included), then the exact order among those few
        kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
        mask = (d2 <= kth[:, None]) & (d2 < np.inf)
        for i, j in enumerate(_rows(d2, mask)):
            j = j[:kk]
            d = _dist(d2[i, j])
            j, d = j[d <= r], d[d <= r]          # (a prefix: the distances ascend)
            idx[a + i, :len(j)] = j
            dist[a + i, :len(j)] = d
            found[a + i] = len(j)
    return idx, dist, found


def radius(static, queries, r, chunk_elems=1 << 23):
    """-> (offsets (m + 1,) int64, index int32, distance float32): query i's neighbours at [offsets[i], offsets[i + 1])."""
    P, Q = _arrays(static, queries)
    m = len(Q)
    r = f32(r)
    assert r >= 0
    counts = np.zeros(m + 1, np.int64)
    idx_parts, dist_parts = [np.zeros(0, np.int32)], [np.zeros(0, f32)]
    step = max(1, chunk_elems // max(1, len(P)))
    for a in range(0, m, step):
        d2 = _d2(P, Q[a:a + step])
        mask = (d2 < np.inf) & (_dist(d2) <= r)   # the predicate itself, on the float32 distance
        for i, j in enumerate(_rows(d2, mask)):
            counts[a + i + 1] = len(j)
            idx_parts.append(j.astype(np.int32))
            dist_parts.append(_dist(d2[i, j]))
    return np.cumsum(counts), np.concatenate(idx_parts), np.concatenate(dist_parts).astype(f32)
