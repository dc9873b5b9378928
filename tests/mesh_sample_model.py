"""numpy model of sdfk_trimesh_sample (include/sdfkit_hip.h "Triangle meshes: sampling"; sdfkit_amd/csrc/trimesh_sample.h): the
integer weights and their exclusive scan, the splitmix draws (uint64 arrays, wrapping), mulhi64 by 32-bit limbs, the plain and the
stratified pick, the fold into exact barycentric weights and every output of a sample."""
from collections import namedtuple

import numpy as np

from tests import meshsdf_model as MM

f32 = np.float32
f64 = np.float64
u64 = np.uint64

GOLDEN = u64(0x9E3779B97F4A7C15)
ONE53 = u64(1) << u64(53)
M32 = u64(0xFFFFFFFF)

Samples = namedtuple("Samples", "Points Normals Colors Triangles Weights w k")


def _u(x):
    return np.asarray(x, u64)


def splitmix(z):
    z = _u(z).copy()
    with np.errstate(over="ignore"):
        z ^= z >> u64(30); z *= u64(0xBF58476D1CE4E5B9)
        z ^= z >> u64(27); z *= u64(0x94D049BB133111EB)
        z ^= z >> u64(31)
    return z


def draws(seed, s):
    """h0, h1, h2 of the samples s (uint64 array)."""
    s = _u(s)
    with np.errstate(over="ignore"):
        return [splitmix(u64(seed) + (u64(3) * s + u64(j + 1)) * GOLDEN) for j in range(3)]


def mulhi64(a, b):
    a, b = np.broadcast_arrays(_u(a), _u(b))
    a0, a1, b0, b1 = a & M32, a >> u64(32), b & M32, b >> u64(32)
    with np.errstate(over="ignore"):
        mid = a1 * b0 + ((a0 * b0) >> u64(32))          # < 2^64
        mid2 = a0 * b1 + (mid & M32)                    # < 2^64
        return a1 * b1 + (mid >> u64(32)) + (mid2 >> u64(32))


def tri_normals(V, T):
    """(n (nt, 3), A2 (nt,)) in binary64, as trimesh_sample.h area2."""
    V = np.asarray(V, f32).reshape(-1, 3).astype(f64)
    T = np.asarray(T, np.int64).reshape(-1, 3)
    a, b, c = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    return tri_normals_abc(a, b, c)


def tri_normals_abc(a, b, c):
    e1, e2 = b - a, c - a
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    return n, (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]


def weight(a2, a2max):
    return (np.sqrt(np.asarray(a2, f64) / f64(a2max)) * 4294967296.0).astype(u64)


def weights(V, T):
    """(w uint64 (nt,), W uint64 (nt + 1,)): W[nt] is the total.  None, None when no triangle has an area."""
    _, a2 = tri_normals(V, T)
    if not a2.max() > 0:
        return None, None
    w = weight(a2, a2.max())
    W = np.zeros(len(w) + 1, u64)
    W[1:] = np.cumsum(w, dtype=u64)
    return w, W


def stratum(s, total, n):
    s, total, n = _u(s), u64(total), u64(n)
    return (total // n) * s + ((total % n) * s) // n


def pick(h0, s, n, total, stratified):
    if not stratified:
        return mulhi64(h0, u64(total))
    lo = stratum(s, total, n)
    return lo + mulhi64(h0, stratum(_u(s) + u64(1), total, n) - lo)


def fold(h1, h2):
    """(k (n, 3) uint64, w (n, 3) float64)."""
    k1, k2 = _u(h1) >> u64(11), _u(h2) >> u64(11)
    over = k1 + k2 > ONE53
    k1, k2 = np.where(over, ONE53 - k1, k1), np.where(over, ONE53 - k2, k2)
    k0 = ONE53 - k1 - k2
    k = np.stack([k0, k1, k2], 1)
    return k, k.astype(f64) * 2.0 ** -53


def sample_on(a, b, c, h1, h2):
    """Triangles (n, 3) float32 each, draws (n,) -> points f32, normals f32, weights f32, w f64, k uint64."""
    a, b, c = [np.asarray(x, f32).astype(f64) for x in (a, b, c)]
    k, w = fold(h1, h2)
    n, a2 = tri_normals_abc(a, b, c)
    P = ((w[:, 0:1] * a + w[:, 1:2] * b) + w[:, 2:3] * c).astype(f32)
    with np.errstate(all="ignore"):
        Nn = (n / np.sqrt(a2)[:, None]).astype(f32)
    return P, Nn, w.astype(f32), w, k


def sample(V, T, n, seed=0, stratified=True, colors=None):
    """What sdfk_trimesh_sample writes for (mesh, n, seed, flags); w (float64) and k (uint64) are the unrounded weights."""
    V = np.asarray(V, f32).reshape(-1, 3)
    T = np.asarray(T, np.int64).reshape(-1, 3)
    _, W = weights(V, T)
    if W is None:
        raise ValueError("no triangle has an area")
    s = np.arange(n, dtype=u64)
    h0, h1, h2 = draws(seed, s)
    r = pick(h0, s, n, W[-1], stratified)
    t = np.searchsorted(W[1:], r, side="right")
    P, Nn, wf, w, k = sample_on(V[T[t, 0]], V[T[t, 1]], V[T[t, 2]], h1, h2)
    cols = None
    if colors is not None:
        C = np.asarray(colors, f32).reshape(-1, 3)
        cols = MM.blend(C[T[t, 0]], C[T[t, 1]], C[T[t, 2]], w)
    return Samples(P, Nn, cols, t.astype(np.int32), wf, w, k)


def stats(V, T):
    w, W = weights(V, T)
    return int(np.count_nonzero(w)), int(W[-1])
