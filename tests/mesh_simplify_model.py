"""The numpy model of sdfk_trimesh_simplify (include/sdfkit_hip.h, "Triangle meshes: simplification"): the function restated with
numpy's own machinery -- the groups are mesh_weld_model's lattice groups, the vertex sets np.unique's first occurrence, the
eigen-solve pointcloud_model.jacobi -- and no sort of its own.  Not a test module.

The arithmetic is float64 from the float32 inputs, one numpy operation per operation of csrc/trimesh_simplify.h, in its order
(numpy's float64 + - * / and sqrt are correctly rounded and never fused), vectorised ACROSS groups, members and corners and
sequential wherever the header is: a sum over `rank` steps adds the rank-th term of every row that has one.  One rounding to
float32 per output component, so the device and the host build of the header equal this bit for bit."""
from collections import namedtuple

import numpy as np

from tests import mesh_weld_model as W
from tests import pointcloud_model as PM

f32, f64, i32, i64, u32, u64 = np.float32, np.float64, np.int32, np.int64, np.uint32, np.uint64

REPRESENTATIVE, CENTROID, QUADRIC = 0, 1, 2
KEEP_DUPLICATES, CANCEL_PAIRS = 1, 2
CHUNK = 32
TRUNCATION = f64(1e-3)
Refused = W.Refused

Simplify = namedtuple("Simplify", "vertex_map vertex_index triangle_index triangles vertices colors merged degenerate duplicates "
                                  "unreferenced passes fallbacks rep groups placed_before_rounding cell_index")


def index_bytes(n):
    top, b = max(int(n) - 1, 0), 0
    while top:
        b, top = b + 1, top >> 8
    return b


def check(cell, placement, flags):
    c = f32(cell)
    if not (c > 0 and np.isfinite(c)):
        raise Refused("cellSize must be finite and greater than 0")
    if placement not in (0, 1, 2):
        raise Refused("unknown placement")
    if flags & ~3:
        raise Refused("unknown flag bits")
    if flags & 3 == 3:
        raise Refused("KEEP_DUPLICATES and CANCEL_PAIRS exclude each other")


# ---- ordered sums ------------------------------------------------------------------------------------------------------------------
def _ranks(owner):
    """owner: ascending row numbers, one per term -> the rank of every term within its row."""
    owner = np.asarray(owner, i64)
    start = np.flatnonzero(np.r_[True, owner[1:] != owner[:-1]]) if len(owner) else np.zeros(0, i64)
    return np.arange(len(owner)) - np.repeat(start, np.diff(np.r_[start, len(owner)]))


def ordered_sum(terms, owner, rows):
    """terms (m, k) float64, owner (m,) ascending: -> (rows, k): every row's terms added one after the other from +0.0."""
    out = np.zeros((rows, terms.shape[1]), f64)
    rank = _ranks(owner)
    for r in range(int(rank.max()) + 1 if len(rank) else 0):
        at = np.flatnonzero(rank == r)
        out[owner[at]] = out[owner[at]] + terms[at]
    return out


def chunked_sum(terms, group, groups):
    """terms (m, k) of the members listed group by group (group ascending, members ascending inside): the header's chunking --
    chunks of CHUNK members summed in order, the chunk sums summed in order."""
    rank = _ranks(group)
    chunk_of_member = rank // CHUNK
    # number the chunks over all groups, in (group, chunk) order
    first = np.r_[True, (group[1:] != group[:-1]) | (chunk_of_member[1:] != chunk_of_member[:-1])] if len(group) else np.zeros(0, bool)
    chunk_id = np.cumsum(first) - 1
    nchunks = int(chunk_id[-1]) + 1 if len(group) else 0
    chunk_sums = ordered_sum(terms, chunk_id, nchunks)
    chunk_group = group[np.flatnonzero(first)]
    return ordered_sum(chunk_sums, chunk_group, groups)


# ---- the mesh's corner lists (the adjacency of the handle) -------------------------------------------------------------------------
def corner_lists(nv, T):
    """-> (inc_start (nv + 1), inc): the corners 3 t + k of every vertex ascending; index-degenerate triangles list none."""
    T = np.asarray(T, i32).reshape(-1, 3)
    live = ~W.degenerate(T)
    corner = np.flatnonzero(np.repeat(live, 3))
    vert = T.reshape(-1)[corner]
    order = np.argsort(vert, kind="stable")
    start = np.zeros(nv + 1, i64)
    np.add.at(start, vert + 1, 1)
    return np.cumsum(start), corner[order]


# ---- placement ---------------------------------------------------------------------------------------------------------------------
def place(V, T, cols, cell, placement, members, group, groups, first):
    """members: the vertices group by group (ascending inside), group: their group (0 .. groups - 1), first: the first member of
    every group.  -> (positions float32, colours float32, fallback bool, position before rounding float64)."""
    zeros = np.zeros((groups, 3), f32)
    if placement == REPRESENTATIVE:
        return V[first].copy(), (cols[first].copy() if cols is not None else zeros), np.zeros(groups, bool), V[first].astype(f64)
    count = np.bincount(group, minlength=groups).astype(f64)[:, None]
    with np.errstate(all="ignore"):
        c = chunked_sum(V[members].astype(f64), group, groups) / count
        colours = (chunked_sum(cols[members].astype(f64), group, groups) / count).astype(f32) if cols is not None else zeros
    if placement == CENTROID:
        return c.astype(f32), colours, np.zeros(groups, bool), c
    # the quadric: one term per (member, corner), members in order, corners in order
    inc_start, inc = corner_lists(len(V), T)
    deg = (inc_start[members + 1] - inc_start[members]).astype(i64)
    term_member = np.repeat(np.arange(len(members)), deg)                       # ascending: the owner of the member sums
    offs = np.arange(len(term_member)) - np.repeat(np.cumsum(deg) - deg, deg)
    tri = T[inc[inc_start[members][term_member] + offs] // 3]
    cc = c[group[term_member]]
    with np.errstate(all="ignore"):
        q0, q1, q2 = (V[tri[:, k]].astype(f64) - cc for k in range(3))
        e1, e2 = q1 - q0, q2 - q0
        n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        d = -((n0 * q0[:, 0] + n1 * q0[:, 1]) + n2 * q0[:, 2])
        terms = np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, d * n0, d * n1, d * n2], 1)
        own = ordered_sum(terms, term_member, len(members))
        Q = chunked_sum(own, group, groups)
        a, v = PM.jacobi([Q[:, k].copy() for k in range(6)])
        l = [a[0][0], a[1][1], a[2][2]]
        lmax = l[0].copy()
        lmax = np.where(l[1] > lmax, l[1], lmax)
        lmax = np.where(l[2] > lmax, l[2], lmax)
        ok = lmax > 0.0
        cut = TRUNCATION * lmax
        nb = [-Q[:, 6], -Q[:, 7], -Q[:, 8]]
        x = [np.zeros(groups), np.zeros(groups), np.zeros(groups)]
        for i in range(3):
            on = l[i] > cut
            s = (v[0][i] * nb[0] + v[1][i] * nb[1]) + v[2][i] * nb[2]
            t = s / l[i]
            for k in range(3):
                x[k] = np.where(on, x[k] + v[k][i] * t, x[k])
        p = c + np.stack(x, 1)
        k = np.floor(V[first].astype(f64) / f64(f32(cell)))
        lo, hi = k * f64(f32(cell)), (k + 1.0) * f64(f32(cell))
        inside = (np.abs(p) < np.inf) & (p >= lo) & (p < hi)
    ok = ok & np.all(inside, axis=1)
    before = np.where(ok[:, None], p, c)
    return before.astype(f32), colours, ~ok, before


# ---- the function ------------------------------------------------------------------------------------------------------------------
def simplify(V, T, colors=None, cell=1.0, placement=QUADRIC, flags=0):
    check(cell, placement, flags)
    V = np.ascontiguousarray(np.asarray(V, f32).reshape(-1, 3))
    T = np.asarray(T, i32).reshape(-1, 3)
    cols = None if colors is None else np.ascontiguousarray(np.asarray(colors, f32).reshape(-1, 3))
    nv, nt = len(V), len(T)
    rep, groups = W.representatives(W.cells(V, cell))
    R = rep[T]
    live = ~W.degenerate(R)
    tkeep = live.copy()
    if not flags & KEEP_DUPLICATES:
        at = np.flatnonzero(live)
        sets, first, counts = np.unique(np.sort(R[at], axis=1), axis=0, return_index=True, return_counts=True) if len(at) else (None, np.zeros(0, i64), np.zeros(0, i64))
        keep = first if not flags & CANCEL_PAIRS else first[counts % 2 == 1]
        tkeep = np.zeros(nt, bool)
        tkeep[at[keep]] = True           # (np.unique's first occurrence: the lowest triangle index of the set)
    used = np.zeros(nv, bool)
    used[R[tkeep].reshape(-1)] = True
    vkeep = (rep == np.arange(nv)) & used
    vnew = np.cumsum(vkeep) - vkeep
    vertex_index = np.flatnonzero(vkeep).astype(i32)
    triangle_index = np.flatnonzero(tkeep).astype(i32)
    vertex_map = np.where(vkeep[rep], vnew[rep], -1).astype(i32)
    triangles = vnew[R[tkeep]].astype(i32).reshape(-1)
    # the kept groups, numbered as the output numbers them; their members ascending
    kv = len(vertex_index)
    member_mask = vkeep[rep]
    members = np.flatnonzero(member_mask)
    group = vnew[rep[members]]
    order = np.argsort(group, kind="stable")
    members, group = members[order], group[order].astype(i64)
    pos, colours, fallback, before = place(V, T, cols, cell, placement, members, group, kv, vertex_index.astype(i64))
    passes = W.passes(V, cell) + (0 if flags & KEEP_DUPLICATES else 3 * index_bytes(groups))
    cell_index = np.floor(V[vertex_index].astype(f64) / f64(f32(cell)))
    return Simplify(vertex_map, vertex_index, triangle_index, triangles, np.ascontiguousarray(pos), np.ascontiguousarray(colours), nv - groups,
                    int(nt - live.sum()), int(live.sum() - tkeep.sum()), groups - kv, passes, int(fallback.sum()), rep, groups, before, cell_index)
