"""The numpy model of sdfk_trimesh_weld (include/sdfkit_hip.h, "Triangle meshes: welding"): the function restated with numpy's own
machinery -- canonical bit keys and np.unique's first occurrence in exact mode, a binary64 floor in lattice mode -- and no sort
of its own.  Everything is an integer decision; the device and the host build of csrc/trimesh_weld.h equal it as bits."""
from collections import namedtuple

import numpy as np

f32, f64, i32, i64, u32, u64 = np.float32, np.float64, np.int32, np.int64, np.uint32, np.uint64

KEEP_DEGENERATE, KEEP_UNREFERENCED = 1, 2
AXIS_SPAN = 2 ** 21

Weld = namedtuple("Weld", "vertex_map vertex_index triangle_index triangles vertices colors merged degenerate unreferenced rep groups")


class Refused(ValueError):
    """What the library answers with SDFK_ERR_INVALID."""


def bits(V):
    return np.ascontiguousarray(V, f32).view(u32)


def canonical(V):
    """(nv, 3) uint32: the bits of the coordinates, -0 mapped to +0."""
    b = bits(np.asarray(V, f32).reshape(-1, 3)).copy()
    b[b == u32(0x80000000)] = 0
    return b


def cells(V, tolerance):
    """(nv, 3) int64: the lattice cell of every vertex less the per-axis least one; Refused when an axis spans 2^21 cells."""
    k = np.floor(np.asarray(V, f32).reshape(-1, 3).astype(f64) / f64(f32(tolerance)))
    kmin, kmax = k.min(axis=0), k.max(axis=0)
    if np.any(~(kmax - kmin < AXIS_SPAN)):
        raise Refused("an axis spans 2^21 cells of the tolerance or more")
    return (k - kmin).astype(i64)


def group_keys(V, tolerance):
    t = f32(tolerance)
    if not (t >= 0 and np.isfinite(t)):
        raise Refused("tolerance must be finite and not negative")
    return canonical(V) if t == 0 else cells(V, t)


def representatives(keys):
    """rep[v] = the lowest index with v's key; and the number of groups."""
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    return first[np.asarray(inverse).reshape(-1)].astype(i32), len(first)


def degenerate(T):
    return (T[:, 0] == T[:, 1]) | (T[:, 1] == T[:, 2]) | (T[:, 0] == T[:, 2])


def weld(V, T, colors=None, tolerance=0.0, flags=0):
    if flags & ~3:
        raise Refused("unknown flag bits")
    V = np.ascontiguousarray(np.asarray(V, f32).reshape(-1, 3))
    T = np.asarray(T, i32).reshape(-1, 3)
    nv = len(V)
    rep, groups = representatives(group_keys(V, tolerance))
    R = rep[T]
    tkeep = np.ones(len(T), bool) if flags & KEEP_DEGENERATE else ~degenerate(R)
    used = np.zeros(nv, bool)
    used[R[tkeep].reshape(-1)] = True
    is_rep = rep == np.arange(nv)
    vkeep = is_rep & (used | bool(flags & KEEP_UNREFERENCED))
    vnew = np.cumsum(vkeep) - vkeep
    vertex_index = np.flatnonzero(vkeep).astype(i32)
    triangle_index = np.flatnonzero(tkeep).astype(i32)
    vertex_map = np.where(vkeep[rep], vnew[rep], -1).astype(i32)
    triangles = vnew[R[tkeep]].astype(i32).reshape(-1)
    cols = np.zeros((len(vertex_index), 3), f32) if colors is None else np.ascontiguousarray(np.asarray(colors, f32).reshape(-1, 3)[vertex_index])
    return Weld(vertex_map, vertex_index, triangle_index, triangles, np.ascontiguousarray(V[vertex_index]), cols, nv - groups,
                len(T) - len(triangle_index), groups - len(vertex_index), rep, groups)


# ---- the passes of the sorts -------------------------------------------------------------------------------------------------------
def pass_mask(diff):
    diff = int(diff)
    return sum(1 << d for d in range(8) if (diff >> (8 * d)) & 255)


def sort_keys(V, tolerance):
    """The 64-bit keys of the sorts, in the order they run: exact mode x, then z above y; lattice mode the packed cell."""
    if f32(tolerance) == 0:
        c = canonical(V).astype(u64)
        return [c[:, 0], c[:, 2] << u64(32) | c[:, 1]]
    k = cells(V, tolerance).astype(u64)
    return [k[:, 2] << u64(42) | k[:, 1] << u64(21) | k[:, 0]]


def passes(V, tolerance):
    """The radix passes run: the bytes in which some two keys differ, over the sorts."""
    return sum(bin(pass_mask(np.bitwise_or.reduce(k ^ k[0]))).count("1") for k in sort_keys(V, tolerance))
