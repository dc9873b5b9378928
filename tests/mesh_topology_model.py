"""numpy model of sdfk_trimesh_components / _topology / _select (include/sdfkit_hip.h, "Triangle meshes: topology"): the
connectivity of a triangle mesh by index.  Labels by vectorised min-hooking plus pointer jumping to the fixpoint (`labels`), a
plain Python union-find for cross-checks on small meshes (`labels_union_find`), the edge census with np.unique on the keys.
Every quantity is an integer; the area weights are those of tests/mesh_sample_model.py."""
from collections import namedtuple

import numpy as np

from tests import mesh_sample_model as SM

i32, i64, u64 = np.int32, np.int64, np.uint64

ROW = ("triangles", "vertices", "edges", "boundary", "non_manifold", "odd", "inconsistent", "area_weight")
CENSUS = ("components", "vertices", "edges", "boundary", "non_manifold", "odd", "inconsistent", "degenerate")

# vertex (nv,) / triangle (nt,) int32 labels, count C, rows (C, 8) int64, census (8,) int64, rounds / shortcuts of the model's own
# label rounds (not the device's: the device may see newer parents within a launch)
Topology = namedtuple("Topology", "vertex triangle count rows census rounds shortcuts")


def _tris(T):
    return np.asarray(T, i64).reshape(-1, 3)


def degenerate(T):
    T = _tris(T)
    return (T[:, 0] == T[:, 1]) | (T[:, 1] == T[:, 2]) | (T[:, 0] == T[:, 2])


def labels(nv, T):
    """(vertex labels, triangle labels, C, hook rounds, shortcut launches): synchronous hook-and-shortcut rounds."""
    T = _tris(T)
    live = T[~degenerate(T)]
    parent = np.arange(nv, dtype=i64)
    rounds = shortcuts = 0
    while True:
        rounds += 1
        assert rounds <= nv + 1
        p = parent[live]                                 # (n, 3): the corners' parents
        m = p.min(axis=1)
        before = parent.copy()
        np.minimum.at(parent, p.reshape(-1), np.repeat(m, 3))
        if np.array_equal(parent, before):
            break
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
            shortcuts += 1
    referenced = np.zeros(nv, bool)
    referenced[live.reshape(-1)] = True
    roots = referenced & (parent == np.arange(nv))
    number = np.cumsum(roots) - roots                    # exclusive: ascending root
    vertex = np.where(referenced, number[parent], -1).astype(i32)
    tri = np.where(degenerate(T), -1, vertex[T[:, 0]]).astype(i32)
    return vertex, tri, int(roots.sum()), rounds, shortcuts


def labels_union_find(nv, T):
    """The same labels by a plain union-find (small meshes only)."""
    T = _tris(T)
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    referenced = [False] * nv
    for a, b, c in T.tolist():
        if a == b or b == c or a == c:
            continue
        for x in (a, b, c):
            referenced[x] = True
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    roots = sorted({find(v) for v in range(nv) if referenced[v]})
    number = {r: k for k, r in enumerate(roots)}
    vertex = np.array([number[find(v)] if referenced[v] else -1 for v in range(nv)], i32).reshape(-1)
    tri = np.array([-1 if (a == b or b == c or a == c) else vertex[a] for a, b, c in T.tolist()], i32).reshape(-1)
    return vertex, tri, len(roots)


def edges(T):
    """(keys uint64, m, f) of the distinct undirected edges, ascending by key."""
    T = _tris(T)
    live = T[~degenerate(T)]
    u = live.reshape(-1)
    v = live[:, [1, 2, 0]].reshape(-1)
    key = (np.minimum(u, v).astype(u64) << u64(32)) | np.maximum(u, v).astype(u64)
    keys, inverse, m = np.unique(key, return_inverse=True, return_counts=True)
    f = np.bincount(inverse.reshape(-1), weights=(u < v), minlength=len(keys)).astype(i64)
    return keys, m.astype(i64), f


def area_weights(V, T):
    """The integer sampling weight of every triangle; zeros when no triangle has an area."""
    w, _ = SM.weights(V, T)
    return np.zeros(len(_tris(T)), i64) if w is None else w.astype(i64)


def topology(V, T):
    V = np.asarray(V, np.float32).reshape(-1, 3)
    T = _tris(T)
    nv = len(V)
    vertex, tri, C, rounds, shortcuts = labels(nv, T)
    keys, m, f = edges(T)
    comp = vertex[(keys >> u64(32)).astype(i64)] if len(keys) else np.zeros(0, i32)
    cols = [np.ones(len(keys), i64), m == 1, m >= 3, m % 2 == 1, (m == 2) & (f != 1)]
    rows = np.zeros((C, 8), i64)
    rows[:, 0] = np.bincount(tri[tri >= 0], minlength=C)
    rows[:, 1] = np.bincount(vertex[vertex >= 0], minlength=C)
    for k, col in enumerate(cols):
        rows[:, 2 + k] = np.bincount(comp, weights=col.astype(i64), minlength=C).astype(i64)
    w = area_weights(V, T)
    np.add.at(rows[:, 7], tri[tri >= 0], w[tri >= 0])   # (int64 adds: a float bincount would round weights of up to 2^32 each)
    census = np.array([C, int((vertex >= 0).sum())] + [int(np.sum(c)) for c in cols] + [int(degenerate(T).sum())], i64)
    return Topology(vertex, tri, C, rows, census, rounds, shortcuts)


def euler(row):
    return int(row[1] - row[2] + row[0])


def watertight(row):
    return int(row[5]) == 0


def oriented(row):
    return int(row[6]) == 0 and int(row[4]) == 0


Selected = namedtuple("Selected", "vertex_index triangle_index triangles vertices colors")


def select(V, T, keep, colors=None, topo=None):
    """keep: C flags.  -> Selected (triangles flat int32, colours zeros when the mesh has none)."""
    V = np.asarray(V, np.float32).reshape(-1, 3)
    T = _tris(T)
    topo = topo or topology(V, T)
    keep = np.asarray(keep).astype(bool).reshape(-1)
    assert len(keep) == topo.count
    kv = (topo.vertex >= 0) & np.append(keep, False)[topo.vertex]
    kt = (topo.triangle >= 0) & np.append(keep, False)[topo.triangle]
    new = np.cumsum(kv) - kv
    vi = np.flatnonzero(kv).astype(i32)
    ti = np.flatnonzero(kt).astype(i32)
    cols = np.zeros((len(vi), 3), np.float32) if colors is None else np.asarray(colors, np.float32).reshape(-1, 3)[vi]
    return Selected(vi, ti, new[T[ti]].astype(i32).reshape(-1), V[vi], cols)


def keep_small_removed(rows, min_triangles=0, min_area_fraction=0.0):
    """RemoveSmallComponents' keep flags."""
    total = int(rows[:, 7].sum())
    return np.array([int(r[0]) >= min_triangles and float(int(r[7])) >= float(min_area_fraction) * float(total) for r in rows], bool)


def largest(rows):
    """LargestComponent's choice (-1: no component): greatest area weight, then more triangles, then the lower number."""
    best = -1
    for c, r in enumerate(rows):
        if best < 0 or (int(r[7]), int(r[0])) > (int(rows[best][7]), int(rows[best][0])):
            best = c
    return best
