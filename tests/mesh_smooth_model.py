"""numpy model of sdfk_trimesh_adjacency / _smooth / _vertex_normals (include/sdfkit_hip.h, "Triangle meshes: adjacency,
smoothing, vertex normals").  binary64 throughout, one float32 rounding at the end of a step or a normal.  The sums keep the
stated order without np.add.at: round k adds the k-th neighbour (corner) of every vertex that has one, so each vertex's own sum
runs first neighbour, second, ... in ascending order, one rounding per add."""
from collections import namedtuple

import numpy as np

f32, f64, i32, i64, u32, u8 = np.float32, np.float64, np.int32, np.int64, np.uint32, np.uint8

# start (nv + 1,) uint32, neighbors (E,) uint32 ascending and unique per vertex, boundary (nv,) uint8, degree (nv,) int64
Adjacency = namedtuple("Adjacency", "start neighbors boundary degree")
# start (nv + 1,) uint32, corners (n,) uint32: 3 t + k, ascending per vertex
Corners = namedtuple("Corners", "start corners")


def _tris(T):
    return np.asarray(T, i64).reshape(-1, 3)


def live(T):
    """The triangles that are not index-degenerate (their indices into T)."""
    T = _tris(T)
    return np.flatnonzero((T[:, 0] != T[:, 1]) & (T[:, 1] != T[:, 2]) & (T[:, 0] != T[:, 2]))


def adjacency(nv, T):
    T = _tris(T)
    L = T[live(T)]
    a, b, c = L[:, 0], L[:, 1], L[:, 2]
    frm = np.stack([a, b, b, c, c, a], 1).reshape(-1)
    to = np.stack([b, a, c, b, a, c], 1).reshape(-1)
    keys, counts = np.unique(frm << 32 | to, return_counts=True)      # ascending: by from, then by to
    v, w = keys >> 32, keys & 0xFFFFFFFF
    degree = np.bincount(v, minlength=nv).astype(i64)
    start = np.zeros(nv + 1, i64)
    start[1:] = np.cumsum(degree)
    boundary = np.zeros(nv, u8)
    boundary[v[counts == 1]] = 1
    boundary[w[counts == 1]] = 1
    return Adjacency(start.astype(u32), w.astype(u32), boundary, degree)


def corners(nv, T):
    T = _tris(T)
    keep = live(T)
    vert = T[keep].reshape(-1)
    corner = (3 * keep[:, None] + np.arange(3)[None, :]).reshape(-1)   # generated in (t, k) order
    order = np.argsort(vert, kind="stable")
    start = np.zeros(nv + 1, i64)
    start[1:] = np.cumsum(np.bincount(vert, minlength=nv))
    return Corners(start.astype(u32), corner[order].astype(u32))


def step(P, adj, s, pinned=None):
    """One step with factor s (a float32): P (nv, 3) float32 -> (nv, 3) float32."""
    P = np.ascontiguousarray(P, f32).reshape(-1, 3)
    start, deg = adj.start.astype(i64)[:-1], adj.degree
    moves = deg > 0
    if pinned is not None:
        moves &= ~np.asarray(pinned, bool)
    D = P.astype(f64)
    acc = np.zeros_like(D)
    first = np.flatnonzero(deg > 0)
    acc[first] = D[adj.neighbors[start[first]]]
    for k in range(1, int(deg.max()) if len(deg) else 0):
        sel = np.flatnonzero(deg > k)
        acc[sel] = acc[sel] + D[adj.neighbors[start[sel] + k]]
    out = P.copy()
    with np.errstate(all="ignore"):
        mean = acc[moves] / deg[moves].astype(f64)[:, None]
        p = D[moves]
        out[moves] = (p + f64(f32(s)) * (mean - p)).astype(f32)
    return out


def smooth(V, T, iterations, lam=0.5, mu=-0.53, pin_boundary=True, adj=None):
    V = np.ascontiguousarray(V, f32).reshape(-1, 3)
    adj = adj or adjacency(len(V), T)
    pinned = adj.boundary != 0 if pin_boundary else None
    P = V.copy()
    for _ in range(iterations):
        P = step(P, adj, lam, pinned)
        if f32(mu) != 0:
            P = step(P, adj, mu, pinned)
    return P


def face_cross(P, T):
    """(b - a) x (c - a) per triangle in binary64, as the sampler's area2 forms it: each product rounded, then one subtraction."""
    P = np.ascontiguousarray(P, f32).reshape(-1, 3).astype(f64)
    T = _tris(T)
    with np.errstate(all="ignore"):
        e1, e2 = P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]]
        return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)


def vertex_normals(P, T, flip=False, cor=None):
    P = np.ascontiguousarray(P, f32).reshape(-1, 3)
    nv = len(P)
    cor = cor or corners(nv, T)
    n = face_cross(P, T)
    start = cor.start.astype(i64)
    deg = start[1:] - start[:-1]
    acc = np.zeros((nv, 3), f64)
    with np.errstate(all="ignore"):
        for k in range(int(deg.max()) if nv else 0):
            sel = np.flatnonzero(deg > k)
            acc[sel] = acc[sel] + n[cor.corners[start[sel] + k] // 3]
        ln = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
        usable = (deg > 0) & (ln > 0) & (ln < np.inf)
        c = acc / ln[:, None]
        out = np.where(usable[:, None], (-c if flip else c).astype(f32), f32(0))
    return np.ascontiguousarray(out, f32)


def side_votes(N, present):
    """(positive, negative): the vertices whose normal has a positive / negative dot product ((x x' + y y') + z z' in binary64)
    with the present one.  Mesh.RecomputeNormals(flip=None) flips iff negative > positive."""
    a, b = np.asarray(N, f32).reshape(-1, 3).astype(f64), np.asarray(present, f32).reshape(-1, 3).astype(f64)
    with np.errstate(all="ignore"):
        d = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    return int(np.count_nonzero(d > 0)), int(np.count_nonzero(d < 0))
