"""The numpy restatement of sdfkit_amd/csrc/trimesh_winding.h (include/sdfkit_hip.h, "Triangle meshes: generalized winding number"):
the hierarchy, the moments, the acceptance test, the walk, the stated atan2 and the order of the sum, bit for bit; and brute(), the
plain sum over all triangles with np.arctan2, which is the yardstick for accuracy only, never for bits.

The walk is run for all queries at once: the nodes are visited in the one depth-first order every query follows, each node for
the queries that opened all of its ancestors, so every query adds its terms in its own walk's order."""
import numpy as np

f32, f64 = np.float32, np.float64

MAX_LEVEL = 6
DIRECT = 4
PI = float.fromhex("0x1.921fb54442d18p+1")
HALF_PI = float.fromhex("0x1.921fb54442d18p+0")
TWO_PI = float.fromhex("0x1.921fb54442d18p+2")
FOUR_PI = float.fromhex("0x1.921fb54442d18p+3")
ATAN_EIGHTH = np.array([float.fromhex(h) for h in (
    "0x0p+0", "0x1.fd5ba9aac2f6ep-4", "0x1.f5b75f92c80ddp-3", "0x1.6f61941e4def1p-2", "0x1.dac670561bb4fp-2", "0x1.1e00babdefeb4p-1",
    "0x1.4978fa3269ee1p-1", "0x1.700a7c5784634p-1", "0x1.921fb54442d18p-1")], f64)
_P = [float.fromhex(h) for h in ("-0x1.5555555555555p-2", "0x1.999999999999ap-3", "-0x1.2492492492492p-3", "0x1.c71c71c71c71cp-4",
                                 "-0x1.745d1745d1746p-4", "0x1.3b13b13b13b14p-4", "-0x1.1111111111111p-4")]


def levels_for(nt):
    L = 0
    while L < MAX_LEVEL and (16 << (2 * L)) < nt:
        L += 1
    return L


def level_offset(l):
    return ((1 << (3 * l)) - 1) // 7


def dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def atan2_64(y, x):
    y, x = np.asarray(y, f64), np.asarray(x, f64)
    with np.errstate(all="ignore"):
        ay, ax = np.abs(y), np.abs(x)
        swap = ay > ax
        t = np.where(swap, ax / ay, ay / ax)
        j = np.rint(t * 8.0)
        u = (t * 8.0 - j) / (8.0 + t * j)
        u2 = u * u
        p = _P[0] + u2 * (_P[1] + u2 * (_P[2] + u2 * (_P[3] + u2 * (_P[4] + u2 * (_P[5] + u2 * _P[6])))))
        a = ATAN_EIGHTH[np.where(np.isfinite(j), j, 0).astype(np.int64)] + (u + (u * u2) * p)
        a = np.where(swap, HALF_PI - a, a)
        a = np.where(x < 0.0, PI - a, a)
        a = np.where(np.isinf(ax) & np.isinf(ay), np.where(x > 0.0, float.fromhex("0x1.921fb54442d18p-1"), float.fromhex("0x1.2d97c7f3321d2p+1")), a)
        r = np.where(y < 0.0, -a, a)
        r = np.where(y == 0.0, np.where(np.signbit(x), np.where(np.signbit(y), -PI, PI), y), r)
        return np.where(np.isnan(x) | np.isnan(y), x + y, r)


def _corners(V, T):
    V = np.asarray(V, f32).reshape(-1, 3)
    T = np.asarray(T, np.int64).reshape(-1, 3)
    return V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]


def triangle_terms(a, b, c, q, atan2=atan2_64):
    """Omega / (4 pi) of the triangles (a, b, c) (f32, broadcast against) the queries q (f64)."""
    A, B, C = a.astype(f64) - q, b.astype(f64) - q, c.astype(f64) - q
    la, lb, lc = np.sqrt(dot3(A, A)), np.sqrt(dot3(B, B)), np.sqrt(dot3(C, C))
    x = np.stack([B[..., 1] * C[..., 2] - B[..., 2] * C[..., 1], B[..., 2] * C[..., 0] - B[..., 0] * C[..., 2],
                  B[..., 0] * C[..., 1] - B[..., 1] * C[..., 0]], -1)
    det = dot3(A, x)
    den = (((la * lb) * lc + dot3(A, B) * lc) + dot3(B, C) * la) + dot3(C, A) * lb
    return atan2(det, den) / TWO_PI


class Tree:
    pass


def build(V, T):
    a, b, c = _corners(V, T)
    nt = len(a)
    H = Tree()
    H.a, H.b, H.c, H.nt = a, b, c, nt
    L = H.L = levels_for(nt)
    lo = np.minimum(np.minimum(a, b), c).min(0)
    hi = np.maximum(np.maximum(a, b), c).max(0)
    ext = float((hi.astype(f64) - lo.astype(f64)).max())
    scale = float(1 << L) / ext if ext > 0 else 0.0
    a64, b64, c64 = a.astype(f64), b.astype(f64), c.astype(f64)
    ctr = ((a64 + b64) + c64) / 3.0
    n = 1 << L
    u = (ctr - lo.astype(f64)) * scale
    k = np.where(u >= n, n - 1, np.where(u > 0.0, np.trunc(np.clip(u, 0, n)), 0)).astype(np.int64)
    code = np.zeros(nt, np.int64)
    for ax in range(3):
        for bit in range(L):
            code |= ((k[:, ax] >> bit) & 1) << (3 * bit + ax)
    H.code, H.lo, H.scale = code, lo, scale
    order = H.order = np.argsort(code, kind="stable")
    total = H.total = level_offset(L + 1)
    first = level_offset(L)
    cells = 1 << (3 * L)
    count, start = np.zeros(total, np.int64), np.zeros(total, np.int64)
    count[first:] = np.bincount(code, minlength=cells)
    start[first:] = np.cumsum(count[first:]) - count[first:]
    # per triangle: n, weight, weight * centroid
    e1, e2 = b64 - a64, c64 - a64
    nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
    w = np.sqrt(dot3(nrm, nrm))
    val = np.concatenate([nrm, w[:, None] * ctr, w[:, None]], 1)[order]      # in sorted order
    S = np.zeros((total, 7), f64)
    for p in range(int(count[first:].max())):
        m = np.flatnonzero(count[first:] > p)
        S[first + m] = S[first + m] + val[start[first + m] + p]
    for l in range(L - 1, -1, -1):
        nodes = level_offset(l) + np.arange(1 << (3 * l))
        for ch in range(8):
            S[nodes] = S[nodes] + S[8 * nodes + 1 + ch]
            count[nodes] += count[8 * nodes + 1 + ch]
        start[nodes] = start[8 * nodes + 1]
    H.count, H.start, H.sums = count, start, S
    occ = count > 0
    H.N = 0.5 * S[:, 0:3]
    firstctr = ctr[order[np.minimum(start, nt - 1)]]
    with np.errstate(all="ignore"):
        H.P = np.where((S[:, 6] > 0.0)[:, None], S[:, 3:6] / S[:, 6:7], firstctr)
    H.N[~occ] = 0
    H.P[~occ] = 0
    r2 = np.zeros(total, f64)
    for l in range(L + 1):
        node = level_offset(l) + (code >> (3 * (L - l)))
        for v in (a, b, c):
            e = v.astype(f64) - H.P[node]
            np.maximum.at(r2, node, dot3(e, e))
    H.r2 = r2
    H.occupied = int(occ.sum())
    H.max_leaf = int(count[first:].max())
    return H


class Result:
    """w (f64), winding (f32), inside (bool), clusters / triangles (int64 per query)"""


def winding(H, Q, beta):
    qf = np.asarray(Q, f32).reshape(-1, 3)
    nq = len(qf)
    q = qf.astype(f64)
    w = np.zeros(nq, f64)
    ncl, ntr = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    beta2 = f64(f32(beta)) * f64(f32(beta))
    finite = np.all(np.isfinite(qf), 1)

    def visit(n, level, idx):
        if H.count[n] == 0 or len(idx) == 0:
            return
        D = H.P[n] - q[idx]
        d2 = dot3(D, D)
        with np.errstate(all="ignore"):
            far = d2 > beta2 * H.r2[n]
        fi = idx[far]
        if len(fi):
            Df, d2f = D[far], d2[far]
            w[fi] = w[fi] + dot3(Df, H.N[n]) / (FOUR_PI * (d2f * np.sqrt(d2f)))
            ncl[fi] += 1
        near = idx[~far]
        if len(near) == 0:
            return
        if level == H.L or H.count[n] <= DIRECT:
            for j in range(H.start[n], H.start[n] + H.count[n]):
                t = H.order[j]
                w[near] = w[near] + triangle_terms(H.a[t], H.b[t], H.c[t], q[near])
            ntr[near] += H.count[n]
        else:
            for ch in range(8):
                visit(8 * n + 1 + ch, level + 1, near)

    visit(0, 0, np.flatnonzero(finite))
    w[~finite] = np.nan
    R = Result()
    R.w, R.clusters, R.triangles = w, ncl, ntr
    with np.errstate(invalid="ignore"):
        R.inside = np.abs(w) > 0.5
        R.winding = np.where(np.isnan(w), f32(np.nan), w.astype(f32)).astype(f32)
    return R


def sorted_brute(H, Q):
    """The stated triangle terms added in sorted order: what beta = +inf walks."""
    q = np.asarray(Q, f32).reshape(-1, 3).astype(f64)
    w = np.zeros(len(q), f64)
    for t in H.order:
        w = w + triangle_terms(H.a[t], H.b[t], H.c[t], q)
    return w


def brute(V, T, Q, chunk=1 << 21):
    """sum over all triangles of 2 np.arctan2(det, den) / (4 pi), binary64: the yardstick for accuracy."""
    a, b, c = _corners(V, T)
    q = np.asarray(Q, f32).reshape(-1, 3).astype(f64)
    out = np.zeros(len(q), f64)
    step = max(1, chunk // max(len(a), 1))
    for s in range(0, len(q), step):
        out[s:s + step] = triangle_terms(a[None], b[None], c[None], q[s:s + step, None, :], atan2=np.arctan2).sum(1)
    return out


def centres(mn, mx, n, z0=0, nz_local=None):
    """The f32 cell centres of a volume (or a slab of it), in the volume pass's order (z fastest)."""
    from tests import meshsdf_model as MM
    nx, ny, nzg = n
    nz = nzg - z0 if nz_local is None else nz_local
    d, m = MM.grid_constants(mn, mx, n)
    I, J, K = [x.reshape(-1) for x in np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")]
    return np.stack([MM.coord(m[0], I, d[0]), MM.coord(m[1], J, d[1]), MM.coord(m[2], z0 + K, d[2])], -1).astype(f32)
