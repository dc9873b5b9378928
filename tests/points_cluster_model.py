"""A numpy model of the KdTree's density clustering (include/sdfkit_hip.h, "Point clouds: clusters"), the yardstick of
sdfkit_amd.points.KdTree.Clusters / SelectClusters (csrc/lib_points_cluster.hip).  Not a test module.

The contract restated on tests/points_knn_model.radius, whose rows are the library's radius query of every static point: within(i, j)
is membership of j in row i, rows are ordered by (d2, index).  Every output is an integer, so the comparison is np.array_equal.
"""
import numpy as np

from tests import points_knn_model as KM

f32 = np.float32
INT32_MAX = np.iinfo(np.int32).max


class Refused(Exception):
    """SDFK_ERR_INVALID"""


def neighbours(points, radius):
    """-> (offsets (n + 1,) int64, index int32): row i = the static points within `radius` of p_i, ascending by (d2, index)."""
    P = np.ascontiguousarray(np.asarray(points, f32).reshape(-1, 3))
    off, idx, _ = KM.radius(P, P, f32(radius))
    return off, idx


def components(n, a, b):
    """The least member of every node's connected component over the directed edges a[e] -> b[e] (a ascending, the edge set
    symmetric); a node without an edge is its own."""
    lab = np.arange(n, dtype=np.int64)
    if not len(a):
        return lab
    starts = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])
    rows = a[starts]
    while True:
        new = lab.copy()
        new[rows] = np.minimum(new[rows], np.minimum.reduceat(lab[b], starts))
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            return lab
        lab = new


def cluster(points, radius, min_points=1, rows=None):
    """-> dict(labels (n,) int32, sizes (C,) int32, core (n,) bool, counts (n,) int32, n_clusters, stats [C, core, border, noise]).
    rows: neighbours(points, radius), when the caller has it already."""
    P = np.ascontiguousarray(np.asarray(points, f32).reshape(-1, 3))
    r = f32(radius)
    if not (r >= 0) or int(min_points) < 1:        # (NaN and negative radii)
        raise Refused
    off, idx = rows if rows is not None else neighbours(P, r)
    n = len(P)
    per = np.diff(off)
    counts = np.minimum(per, INT32_MAX).astype(np.int32)
    core = counts >= int(min_points)
    src = np.repeat(np.arange(n, dtype=np.int64), per)
    dst = idx.astype(np.int64)
    edge = core[src] & core[dst]
    root = components(n, src[edge], dst[edge])
    labels = np.full(n, -1, np.int32)
    roots = np.unique(root[core])                   # ascending: clusters by their lowest core member
    labels[core] = np.searchsorted(roots, root[core])
    # border: the first core entry of the row, rows being in (d2, index) order
    hit = np.flatnonzero(core[dst])
    first = np.full(n, -1, np.int64)
    row, at = np.unique(src[hit], return_index=True)
    first[row] = dst[hit[at]]
    border = ~core & (first >= 0)
    labels[border] = labels[first[border]]
    sizes = np.bincount(labels[labels >= 0], minlength=len(roots)).astype(np.int32)
    return {"labels": labels, "sizes": sizes, "core": core, "counts": counts, "n_clusters": len(roots),
            "stats": [len(roots), int(core.sum()), int(border.sum()), int((labels < 0).sum())]}


def select(labels, keep, n_clusters=None):
    """-> the kept indices, ascending: 0 <= label < n_clusters and keep[label]."""
    labels = np.asarray(labels, np.int32)
    keep = np.asarray(keep).astype(bool).reshape(-1)
    C = len(keep) if n_clusters is None else int(n_clusters)
    if C < 0:
        raise Refused
    ok = (labels >= 0) & (labels < C)
    ok[ok] = keep[labels[ok]]
    return np.flatnonzero(ok).astype(np.int32)


def keep_by_size(sizes, min_size):
    return (np.asarray(sizes) >= int(min_size)).astype(np.uint8)


def largest(sizes):
    """The cluster of greatest size, ties to the lowest number; -1 without clusters."""
    sizes = np.asarray(sizes)
    return int(np.argmax(sizes)) if len(sizes) else -1
