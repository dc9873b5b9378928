"""A numpy model of the consistent orientation of point-cloud normals (include/sdfkit_hip.h, "Point clouds: a consistent
orientation"), the yardstick of sdfkit_amd.points.KdTree.OrientNormals (csrc/lib_orient.hip, csrc/points_orient.h).  Not a test module.

Neighbour rows come from tests/points_knn_model.knn.  The dot is float64 from the float32 inputs, one numpy operation per operation
of points_orient.h, in its order; every decision is a comparison of such values, so the library's signs and stats equal these.
"""
import numpy as np

from tests import points_knn_model as KM

f32 = np.float32
f64 = np.float64
LEVELS = (0.9375, 0.75, 0.5, 0.0)


def valid(Nn):
    """points_orient.h valid: finite and not all zero."""
    Nn = np.asarray(Nn, f32).reshape(-1, 3)
    return np.isfinite(Nn).all(axis=1) & ~(Nn == 0).all(axis=1)


def dot(a, b):
    a, b = np.asarray(a, f32).astype(f64), np.asarray(b, f32).astype(f64)
    with np.errstate(all="ignore"):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def seed_sign(Nn):
    """+1 / -1 per normal: n_z positive; n_z == 0: the component of largest magnitude positive, ties to the lowest axis."""
    Nn = np.asarray(Nn, f32).reshape(-1, 3)
    big, mag = Nn[:, 0].copy(), np.abs(Nn[:, 0])
    for a in (1, 2):
        more = np.abs(Nn[:, a]) > mag
        mag, big = np.where(more, np.abs(Nn[:, a]), mag), np.where(more, Nn[:, a], big)
    by_magnitude = np.where(big < 0, -1, 1)
    return np.where(Nn[:, 2] > 0, 1, np.where(Nn[:, 2] < 0, -1, by_magnitude)).astype(np.int64)


def next_seed(z, candidates):
    """The candidate of greatest z (float32 compare, a NaN counts as -inf), ties to the lowest index; -1 without candidates."""
    c = np.nonzero(candidates)[0]
    if len(c) == 0:
        return -1
    zc = np.asarray(z, f32)[c]
    zc = np.where(np.isnan(zc), f32(-np.inf), zc)
    return int(c[np.nonzero(zc == zc.max())[0][0]])


def next_level(level, count, n_levels=len(LEVELS)):
    """The level of the round after one at `level` that oriented `count` points; n_levels: the growth of this seed is over."""
    return n_levels if level >= n_levels else level + (1 if count == 0 else 0)


def choose(n_i, n_row, stamp_row, sign_row, found, r, threshold):
    """One round's choice for m points at once: n_i (m, 3), their rows' normals (m, k, 3), stamps and signs (m, k), the entries in
    use (m,) -> (accepted (m,) bool, sign (m,) of +-1).  A row entry is a source iff it is in use, valid and 0 < stamp < r; the
    source of greatest |dot| is taken, ties to the first; accepted iff that weight >= threshold."""
    n_row = np.asarray(n_row, f32)
    m, k = stamp_row.shape
    src = (np.arange(k)[None, :] < np.asarray(found)[:, None]) & valid(n_row).reshape(m, k) & (stamp_row > 0) & (stamp_row < r)
    d = dot(np.asarray(n_i, f32)[:, None, :], n_row)
    w = np.where(src, np.abs(d), -1.0)
    best = np.argmax(w, axis=1)                       # the first of the greatest
    rows = np.arange(m)
    accepted = src.any(axis=1) & (w[rows, best] >= threshold)
    signed = d[rows, best] * sign_row[rows, best].astype(f64)
    return accepted, np.where(signed < 0, -1, 1).astype(np.int64)


def orient(static, normals3, k=8, max_distance=np.inf, max_seeds=64, levels=LEVELS, rows=None):
    """sdfk_points_orient_normals -> (normals (n, 3) float32, stats dict).  levels: the thresholds (the contract's four; the tests
    also run the single level (0.0,) to record what the levels buy).  rows: (idx, found) when the caller has them already."""
    P = np.ascontiguousarray(np.asarray(static, f32).reshape(-1, 3))
    Nn = np.ascontiguousarray(np.asarray(normals3, f32).reshape(-1, 3))
    assert Nn.shape == P.shape and 2 <= int(k) <= 64 and int(max_seeds) >= 1 and f32(max_distance) >= 0
    n = len(P)
    idx, found = rows if rows is not None else KM.knn(P, P, k, max_distance)[::2]
    ok = valid(Nn)
    stamp = np.zeros(n, np.int64)
    sign = np.ones(n, np.int64)
    per_level = [0] * max(4, len(levels))
    r = seeds = 0
    while seeds < max_seeds:
        s = next_seed(P[:, 2], ok & (stamp == 0))
        if s < 0:
            break
        r += 1
        seeds += 1
        stamp[s], sign[s] = r, seed_sign(Nn[s:s + 1])[0]
        level = 0
        while level < len(levels):
            r += 1
            c = np.nonzero(ok & (stamp == 0))[0]
            j = np.maximum(idx[c], 0)
            accepted, sg = choose(Nn[c], Nn[j], stamp[j], sign[j], found[c], r, levels[level])
            stamp[c[accepted]], sign[c[accepted]] = r, sg[accepted]     # (after every choice was made: Jacobi)
            per_level[level] += int(accepted.sum())
            level = next_level(level, int(accepted.sum()), len(levels))
    out = Nn.view(np.uint32).copy()
    out[sign < 0] ^= np.uint32(0x80000000)
    stats = {"rounds": r, "seeds": seeds, "flipped": int((sign < 0).sum()), "unreached": int((ok & (stamp == 0)).sum()),
             "invalid": int((~ok).sum()), "levels": per_level}
    return out.view(f32), stats
