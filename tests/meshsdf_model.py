"""numpy model of the triangle-mesh distance (sdfkit_amd/csrc/trimesh_sdf.h, csrc/lib_trimesh.hip): the same binary64
closest-point routine, vectorised brute force over all triangles with ties to the lowest index; orient2d signs exact (an f64
filter, fractions.Fraction where it cannot decide); the same perturbation rule, z_cross formula and colour blend."""
from fractions import Fraction

import numpy as np

f32 = np.float32
f64 = np.float64


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _ratio(n, d):
    with np.errstate(all="ignore"):
        return np.where(d > 0, n / np.where(d > 0, d, 1.0), 0.0)


def _segment(p, a, b):
    ab = b - a
    ap = p - a
    num = _dot(ap, ab)
    den = _dot(ab, ab)
    t = np.where(num <= 0, 0.0, np.where(num >= den, 1.0, _ratio(num, den)))
    cp = a + ab * t[..., None]
    r = p - cp
    return t, cp, _dot(r, r)


def _edges(p, a, b, c):
    t, cp, d2 = _segment(p, a, b)
    w = np.stack([1.0 - t, t, np.zeros_like(t)], -1)
    for (s, e, mk) in ((b, c, lambda t: (np.zeros_like(t), 1.0 - t, t)), (c, a, lambda t: (t, np.zeros_like(t), 1.0 - t))):
        t2, cp2, d22 = _segment(p, s, e)
        better = d22 < d2
        d2 = np.where(better, d22, d2)
        cp = np.where(better[..., None], cp2, cp)
        w = np.where(better[..., None], np.stack(mk(t2), -1), w)
    return d2, cp, w


def closest_on_triangle(p, a, b, c):
    """p, a, b, c: broadcastable (..., 3) float64 -> (d2, cp (..., 3), w (..., 3)), as trimesh_sdf.h closest_on_triangle."""
    p, a, b, c = [np.asarray(x, f64) for x in (p, a, b, c)]
    shape = np.broadcast_shapes(p.shape, a.shape, b.shape, c.shape)
    p, a, b, c = [np.broadcast_to(x, shape) for x in (p, a, b, c)]
    ab, ac, ap, bp, cq = b - a, c - a, p - a, p - b, p - c
    n0 = ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1]
    n1 = ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2]
    n2 = ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]
    area = (n0 * n0 + n1 * n1) + n2 * n2
    d1, d2_, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cq), _dot(ac, cq)
    vc = d1 * d4 - d3 * d2_
    vb = d5 * d2_ - d1 * d6
    va = d3 * d6 - d5 * d4
    conds = [(d1 <= 0) & (d2_ <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2_ >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    region = np.select(conds, [0, 1, 2, 3, 4, 5], 6)
    z = np.zeros(shape[:-1])
    u, v, w = np.ones(shape[:-1]), z.copy(), z.copy()
    u = np.where(region == 1, 0.0, u); v = np.where(region == 1, 1.0, v)
    r2 = _ratio(d1, d1 - d3)
    v = np.where(region == 2, r2, v); u = np.where(region == 2, 1.0 - r2, u)
    u = np.where(region == 3, 0.0, u); w = np.where(region == 3, 1.0, w)
    r4 = _ratio(d2_, d2_ - d6)
    w = np.where(region == 4, r4, w); u = np.where(region == 4, 1.0 - r4, u)
    e = d4 - d3
    r5 = _ratio(e, e + (d5 - d6))
    w = np.where(region == 5, r5, w); u = np.where(region == 5, 0.0, u); v = np.where(region == 5, 1.0 - r5, v)
    s = (va + vb) + vc
    face_ok = (va >= 0) & (vb >= 0) & (vc >= 0) & (s > 0)
    with np.errstate(all="ignore"):
        vf, wf = vb / np.where(s > 0, s, 1.0), vc / np.where(s > 0, s, 1.0)
    isf = region == 6
    v = np.where(isf, vf, v); w = np.where(isf, wf, w); u = np.where(isf, (1.0 - vf) - wf, u)
    gen = (a + ab * v[..., None]) + ac * w[..., None]
    q = np.where((region == 0)[..., None], a, np.where((region == 1)[..., None], b, np.where((region == 3)[..., None], c,
                 np.where((region == 5)[..., None], b + (c - b) * w[..., None], gen))))
    r = p - q
    d2 = _dot(r, r)
    W = np.stack([u, v, w], -1)
    use_edges = (area == 0) | (isf & ~face_ok)
    if np.any(use_edges):
        ed2, ecp, ew = _edges(p, a, b, c)
        d2 = np.where(use_edges, ed2, d2)
        q = np.where(use_edges[..., None], ecp, q)
        W = np.where(use_edges[..., None], ew, W)
    return d2, q, W


def closest(V, T, Q, chunk=1 << 22):
    """Brute force: for each query the triangle of least d2 (ties: lowest index) -> (tri int32, dist f32, cp f32, w f64, d2 f64)."""
    V = np.asarray(V, f32).reshape(-1, 3).astype(f64)
    T = np.asarray(T, np.int64).reshape(-1, 3)
    Q = np.asarray(Q, f32).reshape(-1, 3).astype(f64)
    A, B, Cc = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    lo, hi = np.minimum(np.minimum(A, B), Cc), np.maximum(np.maximum(A, B), Cc)
    nq, nt = len(Q), len(T)
    tri = np.empty(nq, np.int32)
    D2 = np.empty(nq)
    CP = np.empty((nq, 3))
    Wt = np.empty((nq, 3))
    if nt * 1 <= 4096:
        per = max(1, chunk // max(nt, 1))
        for s in range(0, nq, per):
            p = Q[s:s + per, None, :]
            d2, cp, w = closest_on_triangle(p, A[None], B[None], Cc[None])
            k = np.argmin(d2, axis=1)
            r = np.arange(len(k))
            tri[s:s + per], D2[s:s + per], CP[s:s + per], Wt[s:s + per] = k, d2[r, k], cp[r, k], w[r, k]
    else:
        for i in range(nq):   # prefilter: only triangles whose AABB is within the nearest vertex distance can win
            p = Q[i]
            ub = np.min(_dot(A - p, A - p)) * (1 + 1e-9)
            g = np.maximum(np.maximum(lo - p, p - hi), 0.0)
            cand = np.nonzero(_dot(g, g) * (1 - 1e-9) <= ub)[0]
            d2, cp, w = closest_on_triangle(p[None], A[cand], B[cand], Cc[cand])
            k = np.argmin(d2)   # (cand ascending: the first minimum is the lowest index)
            tri[i], D2[i], CP[i], Wt[i] = cand[k], d2[k], cp[k], w[k]
    dist = np.sqrt(D2).astype(f32)
    return tri, dist, CP.astype(f32), Wt, D2


# ---- exact orientation --------------------------------------------------------------------------------------------------
def orient_terms(ax, ay, bx, by, px, py):
    ax, ay, bx, by, px, py = [np.asarray(x, f32).astype(f64) for x in (ax, ay, bx, by, px, py)]
    return [bx * py, -(bx * ay), -(ax * py), -(by * px), by * ax, ay * px]


def orient2d_exact(ax, ay, bx, by, px, py):
    """The exact sign of (bx - ax)(py - ay) - (by - ay)(px - ax) on f32 inputs (arrays): an f64 filter, Fraction otherwise."""
    t = orient_terms(ax, ay, bx, by, px, py)
    naive = ((((t[0] + t[1]) + t[2]) + t[3]) + t[4]) + t[5]
    mag = sum(np.abs(x) for x in t)
    sign = np.sign(naive).astype(np.int64)
    unsure = np.abs(naive) <= mag * 2.0 ** -48
    idx = np.nonzero(np.atleast_1d(unsure))[0]
    sign = np.atleast_1d(sign).copy()
    tt = [np.atleast_1d(np.broadcast_to(x, np.shape(naive))) for x in t]
    for i in idx:
        s = sum(Fraction(float(x[i])) for x in tt)
        sign[i] = (s > 0) - (s < 0)
    return sign if np.ndim(naive) else int(sign[0])


def orient2d_fraction(ax, ay, bx, by, px, py):
    """Scalar reference: the sign computed entirely in Fractions of the f32 values."""
    F = [Fraction(float(f32(x))) for x in (ax, ay, bx, by, px, py)]
    s = (F[2] - F[0]) * (F[5] - F[1]) - (F[3] - F[1]) * (F[4] - F[0])
    return (s > 0) - (s < 0)


def orient2d_perturbed(ax, ay, bx, by, px, py):
    s = orient2d_exact(ax, ay, bx, by, px, py)
    ax, ay, bx, by = [np.asarray(x, f32) for x in (ax, ay, bx, by)]
    e1 = np.where(by != ay, np.where(by < ay, 1, -1), np.where(bx != ax, np.where(bx > ax, 1, -1), 0))
    return np.where(s != 0, s, e1)


def _edge_f64(a, b, px, py):
    return (b[..., 0].astype(f64) - a[..., 0].astype(f64)) * (py - a[..., 1].astype(f64)) - \
           (b[..., 1].astype(f64) - a[..., 1].astype(f64)) * (px - a[..., 0].astype(f64))


def z_cross(a, b, c, area, px, py):
    x, y = np.asarray(px, f32).astype(f64), np.asarray(py, f32).astype(f64)
    sg = np.where(area > 0, 1.0, -1.0)
    wa = np.maximum(_edge_f64(b, c, x, y) * sg, 0.0)
    wb = np.maximum(_edge_f64(c, a, x, y) * sg, 0.0)
    wc = np.maximum(_edge_f64(a, b, x, y) * sg, 0.0)
    wa, wb, wc = [np.where(w > 0, w, 0.0) for w in (wa, wb, wc)]
    s = (wa + wb) + wc
    with np.errstate(all="ignore"):
        z = (((wa * a[..., 2].astype(f64)) + (wb * b[..., 2].astype(f64))) + (wc * c[..., 2].astype(f64))) / np.where(s > 0, s, 1.0)
    return np.where(s > 0, z, a[..., 2].astype(f64))


def blend(ca, cb, cc, w):
    wa, wb, wc = [np.asarray(w[..., k], f64).astype(f32)[..., None] for k in range(3)]
    return (ca * wa + cb * wb) + cc * wc


# ---- volumes ------------------------------------------------------------------------------------------------------------
def grid_constants(mn, mx, n):
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    d = np.array([f32(mx[k] - mn[k]) / f32(n[k]) for k in range(3)], f32)
    m = np.array([mn[k] + f32(f32(0.5) * d[k]) for k in range(3)], f32)
    return d, m


def coord(m, i, d):
    return f32(m) + np.asarray(i, np.int64).astype(f32) * f32(d)


def crossings(V, T, m, d, nx, ny):
    """Crossing records (column = i * ny + j, z) of every triangle over the columns of its xy box."""
    V = np.asarray(V, f32).reshape(-1, 3)
    T = np.asarray(T, np.int64).reshape(-1, 3)
    A, B, Cc = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    area = orient2d_exact(A[:, 0], A[:, 1], B[:, 0], B[:, 1], Cc[:, 0], Cc[:, 1])
    xs, ys = coord(m[0], np.arange(nx), d[0]), coord(m[1], np.arange(ny), d[1])
    lo, hi = np.minimum(np.minimum(A, B), Cc), np.maximum(np.maximum(A, B), Cc)
    i0, i1 = np.searchsorted(xs, lo[:, 0], "left"), np.searchsorted(xs, hi[:, 0], "right") - 1
    j0, j1 = np.searchsorted(ys, lo[:, 1], "left"), np.searchsorted(ys, hi[:, 1], "right") - 1
    ni, nj = np.maximum(i1 - i0 + 1, 0), np.maximum(j1 - j0 + 1, 0)
    cnt = np.where(area != 0, ni * nj, 0)
    t = np.repeat(np.arange(len(T)), cnt)
    k = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    i = i0[t] + k % np.maximum(ni[t], 1)
    j = j0[t] + k // np.maximum(ni[t], 1)
    px, py = xs[i], ys[j]
    a, b, c, ar = A[t], B[t], Cc[t], area[t]
    inside = (orient2d_perturbed(a[:, 0], a[:, 1], b[:, 0], b[:, 1], px, py) == ar) & \
             (orient2d_perturbed(b[:, 0], b[:, 1], c[:, 0], c[:, 1], px, py) == ar) & \
             (orient2d_perturbed(c[:, 0], c[:, 1], a[:, 0], a[:, 1], px, py) == ar)
    s = np.nonzero(inside)[0]
    return i[s] * ny + j[s], z_cross(a[s], b[s], c[s], ar[s], px[s], py[s])


def volume(V, T, mn, mx, n, colors=None, band=np.inf, z0=0, nz_local=None, sample=None):
    """Signed distances (and colours) at the cell centres of the volume (min, max, n = (nx, ny, nz_global)), slab planes
    [z0, z0 + nz_local).  sample: an (m, 3) array of local voxel indices -> flat results for those voxels; else full arrays."""
    nx, ny, nzg = n
    nz = nzg - z0 if nz_local is None else nz_local
    d, m = grid_constants(mn, mx, n)
    col, zc = crossings(V, T, m, d, nx, ny)
    if sample is None:
        I, J, Kk = [a.reshape(-1) for a in np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")]
    else:
        I, J, Kk = [np.asarray(sample)[:, a] for a in range(3)]
    zk = coord(m[2], z0 + Kk, d[2])
    P = np.stack([coord(m[0], I, d[0]), coord(m[1], J, d[1]), zk], -1)
    tri, dist, cp, W, D2 = closest(V, T, P)
    # parity: crossings of the voxel's column below its centre
    order = np.argsort(col, kind="stable")
    col, zc = col[order], zc[order]
    qc = I * ny + J
    s0, s1 = np.searchsorted(col, qc, "left"), np.searchsorted(col, qc, "right")
    inside = np.zeros(len(qc), bool)
    zkd = zk.astype(f64)
    for q in np.nonzero(s1 > s0)[0]:
        inside[q] = (np.count_nonzero(zc[s0[q]:s1[q]] < zkd[q]) & 1) == 1
    band = f32(band)
    clamped = dist > band
    dd = np.where(clamped, band, dist)
    val = np.where(inside, -dd, dd).astype(f32)
    rgb = np.zeros((len(val), 3), f32)
    if colors is not None:
        Cv = np.asarray(colors, f32).reshape(-1, 3)
        Tt = np.asarray(T, np.int64).reshape(-1, 3)[tri]
        rgb = blend(Cv[Tt[:, 0]], Cv[Tt[:, 1]], Cv[Tt[:, 2]], W).astype(f32)
        rgb[clamped] = 0
    if sample is None:
        return val.reshape(nx, ny, nz), rgb.reshape(nx, ny, nz, 3)
    return val, rgb


# ---- meshes -------------------------------------------------------------------------------------------------------------
def box_mesh(lo, hi):
    """The 12-triangle axis-aligned box [lo, hi], outward-facing."""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    V = np.array([[lo[0] if i & 1 == 0 else hi[0], lo[1] if i & 2 == 0 else hi[1], lo[2] if i & 4 == 0 else hi[2]] for i in range(8)], f32)
    T = np.array([0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5], np.int32)
    return V, T


def octahedron(center, r):
    c = np.asarray(center, f32)
    V = np.array([c + [r, 0, 0], c - [r, 0, 0], c + [0, r, 0], c - [0, r, 0], c + [0, 0, r], c - [0, 0, r]], f32)
    T = np.array([0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5], np.int32)
    return V, T
