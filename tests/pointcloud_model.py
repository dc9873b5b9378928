"""A numpy model of point-cloud normals and point clouds as signed distance volumes (include/sdfkit_hip.h, "Point clouds: normals
and volumes"), the yardstick of sdfkit_amd.points.KdTree.EstimateNormals / ToVoxels (csrc/lib_pointcloud.hip,
csrc/points_normals.h).  Not a test module.

Neighbours come from tests/points_knn_model.knn.  Everything after them is float64 from the float32 inputs, one numpy operation per
operation of points_normals.h, in its order (numpy's float64 + - * / and sqrt are correctly rounded and never fused), and one
rounding to float32 per result -- so the library's results equal these bit for bit.
"""
import numpy as np

from tests import points_knn_model as KM

f32 = np.float32
f64 = np.float64
FLT_MAX = KM.FLT_MAX
SWEEPS = 8


def radius_d2_bound(r):
    """points_knn.h radius_d2_bound: the largest finite float32 d2 whose correctly rounded root does not exceed r."""
    r = f32(r)
    root = lambda t: f32(np.sqrt(f64(t)))
    rr = f64(r) * f64(r)
    t = FLT_MAX if rr >= f64(FLT_MAX) else f32(rr)
    while t > 0 and root(t) > r:
        t = np.nextafter(t, f32(0))
    while t < FLT_MAX and root(np.nextafter(t, f32(np.inf))) <= r:
        t = np.nextafter(t, f32(np.inf))
    return f32(t)


def _d2(P, Q, idx):
    """The float32 d2 of (Q[i], P[idx[i, j]]), the search's formula; garbage where idx < 0."""
    p = P[np.maximum(idx, 0)]
    dx, dy, dz = Q[:, None, 0] - p[..., 0], Q[:, None, 1] - p[..., 1], Q[:, None, 2] - p[..., 2]
    return (dx * dx + dy * dy) + dz * dz


# ---- normals ----
def covariance(P, idx, found):
    """-> (six float64 arrays c00 c01 c02 c11 c12 c22, trace): the sums of points_normals.h over each row's first `found` neighbours."""
    P64 = P.astype(f64)
    n, k = idx.shape
    q = P64[np.maximum(idx, 0)] - P64[:, None, :]                 # (n, k, 3)
    valid = np.arange(k)[None, :] < found[:, None]
    s = np.zeros((n, 3))
    for j in range(k):
        s = s + np.where(valid[:, j, None], q[:, j], 0.0)
    with np.errstate(all="ignore"):
        mean = s / found.astype(f64)[:, None]
    mean = np.where(found[:, None] > 0, mean, 0.0)
    c = [np.zeros(n) for _ in range(6)]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for j in range(k):
        d = q[:, j] - mean
        for e, (a, b) in enumerate(pairs):
            c[e] = c[e] + np.where(valid[:, j], d[:, a] * d[:, b], 0.0)
    return c, (c[0] + c[3]) + c[5]


def jacobi(c):
    """Cyclic Jacobi of points_normals.h on n symmetric 3x3 at once -> (a: 3x3 list of arrays, v: 3x3 list of arrays)."""
    n = len(c[0])
    a = [[None] * 3 for _ in range(3)]
    a[0][0], a[0][1], a[0][2], a[1][1], a[1][2], a[2][2] = [x.copy() for x in c]
    a[1][0], a[2][0], a[2][1] = a[0][1], a[0][2], a[1][2]
    v = [[np.full(n, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = a[p][q]
                on = apq != 0.0
                theta = (a[q][q] - a[p][p]) / (2.0 * apq)
                at = np.where(theta < 0.0, -theta, theta)
                t = 1.0 / (at + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                app = a[p][p] - t * apq
                aqq = a[q][q] + t * apq
                arp = cs * a[r][p] - sn * a[r][q]
                arq = sn * a[r][p] + cs * a[r][q]
                a[p][p] = np.where(on, app, a[p][p])
                a[q][q] = np.where(on, aqq, a[q][q])
                a[p][q] = a[q][p] = np.where(on, 0.0, apq)
                a[r][p] = a[p][r] = np.where(on, arp, a[r][p])
                a[r][q] = a[q][r] = np.where(on, arq, a[r][q])
                for k in range(3):
                    vkp = cs * v[k][p] - sn * v[k][q]
                    vkq = sn * v[k][p] + cs * v[k][q]
                    v[k][p], v[k][q] = np.where(on, vkp, v[k][p]), np.where(on, vkq, v[k][q])
    return a, v


def normals_from_neighbours(P, idx, found, viewpoint=None):
    """Steps 2-6 of sdfk_points_normals for given knn rows -> (normals (n, 3) float32, variation (n,) float32)."""
    P = np.ascontiguousarray(np.asarray(P, f32).reshape(-1, 3))
    n = len(P)
    c, trace = covariance(P, idx, found)
    a, v = jacobi(c)
    lmin = a[0][0].copy()
    col = np.zeros(n, np.int64)
    for j in (1, 2):
        less = a[j][j] < lmin
        col = np.where(less, j, col)
        lmin = np.where(less, a[j][j], lmin)
    nv = np.stack([np.where(col == 0, v[k][0], np.where(col == 1, v[k][1], v[k][2])) for k in range(3)], axis=1)
    with np.errstate(all="ignore"):
        length = np.sqrt((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2])
        nv = nv / length[:, None]
        big, mag = nv[:, 0].copy(), np.where(nv[:, 0] < 0.0, -nv[:, 0], nv[:, 0])
        for k in (1, 2):
            ma = np.where(nv[:, k] < 0.0, -nv[:, k], nv[:, k])
            more = ma > mag
            mag, big = np.where(more, ma, mag), np.where(more, nv[:, k], big)
        flip = big < 0.0
        if viewpoint is not None:
            w = np.broadcast_to(np.asarray(viewpoint, f32).reshape(-1, 3), (n, 3)).astype(f64)
            P64 = P.astype(f64)
            d = ((w[:, 0] - P64[:, 0]) * nv[:, 0] + (w[:, 1] - P64[:, 1]) * nv[:, 1]) + (w[:, 2] - P64[:, 2]) * nv[:, 2]
            flip = np.where((d < 0.0) | (d > 0.0), d < 0.0, flip)
        nv = np.where(flip[:, None], -nv, nv)
        variation = np.where(lmin < 0.0, 0.0, lmin) / ((a[0][0] + a[1][1]) + a[2][2])   # (a negative l_min is rounding noise: +0.0)
    degenerate = (found < 3) | (trace == 0.0)
    normals = np.where(degenerate[:, None], 0.0, nv).astype(f32)
    return normals, np.where(degenerate, 0.0, variation).astype(f32)


def normals(static, k, viewpoint=None, max_distance=np.inf):
    """sdfk_points_normals -> (normals (n, 3) float32, variation (n,) float32)."""
    assert 3 <= int(k) <= 64
    P = np.ascontiguousarray(np.asarray(static, f32).reshape(-1, 3))
    idx, _, found = KM.knn(P, P, k, max_distance)
    return normals_from_neighbours(P, idx, found, viewpoint)


# ---- volumes ----
def centres(mn, mx, shape):
    """The float32 cell centres (nvox, 3), z fastest: first centre min + 0.5 d, then + i d, d = (max - min) / n."""
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    ax = []
    for a in range(3):
        d = f32((mx[a] - mn[a]) / f32(shape[a]))
        m0 = f32(mn[a] + f32(f32(0.5) * d))
        ax.append((m0 + np.arange(shape[a]).astype(f32) * d).astype(f32))
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)


def blend(P, N, Q, idx, found, k, max_distance):
    """Steps 1-3 of sdfk_points_to_volume for given knn rows of the points Q -> (value float32 (clamped; garbage where unknown), known)."""
    md = f32(max_distance)
    m = len(Q)
    d2 = _d2(P, Q, idx)
    h2 = np.where(found == k, d2[:, k - 1], radius_d2_bound(md)).astype(f32)
    zero_n = (N[:, 0] == 0) & (N[:, 1] == 0) & (N[:, 2] == 0)
    P64, N64, Q64 = P.astype(f64), N.astype(f64), Q.astype(f64)
    S, W, first = np.zeros(m), np.zeros(m), np.zeros(m)
    seen = np.zeros(m, bool)
    blendable = h2 > 0
    with np.errstate(all="ignore"):
        for j in range(k):
            i = np.maximum(idx[:, j], 0)
            valid = (j < found) & ~zero_n[i]
            p, nr = P64[i], N64[i]
            e = ((Q64[:, 0] - p[:, 0]) * nr[:, 0] + (Q64[:, 1] - p[:, 1]) * nr[:, 1]) + (Q64[:, 2] - p[:, 2]) * nr[:, 2]
            first = np.where(valid & ~seen, e, first)
            seen |= valid
            t = d2[:, j].astype(f64) / h2.astype(f64)
            u = 1.0 - t
            w = u * u
            use = valid & blendable
            S = S + np.where(use, w * e, 0.0)
            W = W + np.where(use, w, 0.0)
        value = np.where(W > 0.0, S / np.where(W > 0.0, W, 1.0), first).astype(f32)
    value = np.where(value > md, md, value)
    value = np.where(value < -md, -md, value)
    return value.astype(f32), seen


def fill_signs(sgn):
    """Step 4: sgn (nx, ny, nz) of 0 (unknown) / +-1 -> every entry +-1.  Along z, then y, then x: an unknown entry takes the last
    sign before it on its line, the leading ones the first sign after them; lines without a sign wait for the next pass; a
    volume without any becomes +1."""
    s = np.array(sgn, np.int8)
    for axis in (2, 1, 0):
        t = np.moveaxis(s, axis, -1)                  # a view: written through
        has = (t != 0).any(-1)
        first = np.argmax(t != 0, axis=-1)
        carry = np.take_along_axis(t, first[..., None], -1)[..., 0]
        for i in range(t.shape[-1]):
            cur = t[..., i]
            carry = np.where(cur != 0, cur, carry)
            t[..., i] = np.where(has, carry, cur)
    s[s == 0] = 1
    return s


def to_volume(static, normals3, mn, mx, shape, k=8, max_distance=np.inf):
    """sdfk_points_to_volume -> (values (nx, ny, nz) float32, known (nx, ny, nz) bool)."""
    assert 1 <= int(k) <= 64 and f32(max_distance) > 0
    P = np.ascontiguousarray(np.asarray(static, f32).reshape(-1, 3))
    N = np.ascontiguousarray(np.asarray(normals3, f32).reshape(-1, 3))
    assert N.shape == P.shape
    Q = centres(mn, mx, shape)
    idx, _, found = KM.knn(P, Q, k, max_distance)
    value, known = blend(P, N, Q, idx, found, int(k), max_distance)
    sgn = np.where(known, np.where(value < 0, -1, 1), 0).astype(np.int8).reshape(shape)
    filled = fill_signs(sgn)
    far = np.where(filled < 0, -f32(max_distance), f32(max_distance)).astype(f32)
    return np.where(known.reshape(shape), value.reshape(shape), far).astype(f32), known.reshape(shape)
