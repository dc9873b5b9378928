"""The meshes of the simplification tests (tests/test_mesh_simplify_host.py, tests/test_gpu_mesh_simplify.py,
tests/test_gpu_mesh_simplify_cpp.py) and the recorded results the C++ suite reads (tests/golden/mesh_simplify_cases.json).  A case
is (V (nv, 3) float32, T (nt, 3) int32, colors (nv, 3) float32 or None, cellSize).  Coordinates are small decimals, exact
midpoints of them, or draws of numpy's seeded generator: the same bits on every machine.

    python -m tests.mesh_simplify_cases --record      rewrites the fixture from the model
"""
import json
import os
import sys

import numpy as np

from tests import mesh_topology_cases as TC
from tests import mesh_weld_cases as WC
from tests import mesh_weld_model as W
from tests.mesh_topology_cases import patch, permuted, tetrahedron, torus, zigzag  # noqa: F401
from tests.mesh_weld_cases import index_colors, soup  # noqa: F401

f32, f64, i32, i64, u32 = np.float32, np.float64, np.int32, np.int64, np.uint32
ROOT = TC.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "mesh_simplify_cases.json")
MOVED = WC.MOVED
PLACEMENTS = (0, 1, 2)          # SDFK_SIMPLIFY_REPRESENTATIVE, _CENTROID, _QUADRIC
FLAGS = (0, 1, 2)               # one of each set, SDFK_SIMPLIFY_KEEP_DUPLICATES, SDFK_SIMPLIFY_CANCEL_PAIRS
CHUNK = 32                      # points_filter.h kChunk
TILE = 2048                     # device_sort.h kSortTile


def subdivide(V, T):
    """Every triangle cut into four at its edge midpoints ((a + b) / 2 in float32: exact or one rounding, the same everywhere)."""
    V, T = np.asarray(V, f32), np.asarray(T, i32).reshape(-1, 3)
    mid, pts, out = {}, [tuple(p) for p in V], []

    def m(a, b):
        k = (min(a, b), max(a, b))
        if k not in mid:
            mid[k] = len(pts)
            pts.append(tuple((V[k[0]] + V[k[1]]) / f32(2)))
        return mid[k]

    for a, b, c in T.tolist():
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return np.array(pts, f32), np.array(out, i32)


def box(n, lo, hi):
    """The closed surface of the box [lo, hi], n[a] quads along axis a, outward wound, welded: watertight and oriented."""
    g = [np.array([lo[a] + (hi[a] - lo[a]) * i / n[a] for i in range(n[a] + 1)], f64).astype(f32) for a in range(3)]
    P, T = [], []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            for i in range(n[u]):
                for j in range(n[v]):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0.0, 0.0, 0.0]
                        p[axis], p[u], p[v] = g[axis][-1 if side else 0], g[u][i + di], g[v][j + dj]
                        q.append(p)
                    if not side:
                        q = [q[0], q[3], q[2], q[1]]   # (the other way round from the same corner: opposite faces share their diagonals)
                    b = len(P)
                    P += q
                    T += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
    w = W.weld(np.array(P, f32), np.array(T, i32))
    return w.vertices, w.triangles.reshape(-1, 3)


def concat(*meshes):
    off, Vs, Ts = 0, [], []
    for V, T in meshes:
        Vs.append(np.asarray(V, f32))
        Ts.append(np.asarray(T, i32).reshape(-1, 3) + off)
        off += len(V)
    return np.ascontiguousarray(np.concatenate(Vs)), np.concatenate(Ts).astype(i32)


def fine_torus():
    return subdivide(*subdivide(*torus()))


def nested_shells():
    """A box inside a box, the inner one wound inward: the boundary of a thick shell."""
    Vo, To = box((6, 5, 4), (-1.0, -1.0, -1.0), (2.0, 1.5, 1.0))
    Vi, Ti = box((4, 4, 3), (-0.55, -0.45, -0.6), (1.45, 1.05, 0.55))
    return concat((Vo, To), (Vi, Ti[:, ::-1]))


def thin_slab():
    """A closed slab 0.05 thick: under a cell of 0.25 its two sides collapse onto each other, triangle on triangle, wound against
    each other -- what SDFK_SIMPLIFY_CANCEL_PAIRS removes and the default rule leaves as a one-sided sheet."""
    return box((12, 10, 1), (0.02, 0.03, 0.1), (2.96, 2.47, 0.15))


def flat_patch():
    """A plane z = 0.25 x + 0.125: every group's A has rank 1, and the truncation decides."""
    V, T = patch(12, 10)
    V = V.copy()
    V[:, 2] = f32(0.25) * V[:, 0] + f32(0.125)
    return V, T


def crease():
    """Two planes that meet in the line x = 1.5 (z = |x - 1.5| / 2), extruded along y: rank 2 in the cells of the crease."""
    V, T = patch(12, 10)
    V = V.copy()
    V[:, 2] = np.abs(V[:, 0] - f32(1.5)) * f32(0.5)
    return V, T


def corner():
    """A finely cut box: the cells of its eight corners see three planes (rank 3), those of its edges two, the rest one."""
    return box((9, 9, 9), (0.1, 0.1, 0.1), (2.35, 2.35, 2.35))


def two_sheets():
    """Two sheets over [0, 3) x [0, 3) that share cells and no vertex: z = 0.2 and z = 0.3 + 0.2 x.  Their planes meet in the line
    x = -0.5, outside every cell of the lattice 1: every group's minimiser leaves its cell and falls back to the centroid."""
    V, T = patch(11, 11)
    A = np.stack([V[:, 0] * f32(0.5) + f32(0.125), V[:, 1] + f32(0.0625), np.full(len(V), 0.2, f32)], 1).astype(f32)
    B = A.copy()
    B[:, 2] = f32(0.3) + f32(0.2) * A[:, 0]
    return concat((A, T), (B, T))


def group_sizes(sizes=(1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1), seed=5):
    """One group of each size, cell 1, in the cells (2 i, 0, 0); every member is a corner of a triangle to the two next groups."""
    rng = np.random.default_rng(seed)
    start = np.cumsum([0] + list(sizes))
    V = np.concatenate([np.array([2 * i, 0, 0], f64) + rng.uniform(0.05, 0.95, (s, 3)) for i, s in enumerate(sizes)]).astype(f32)
    T, n = [], len(sizes)
    for i, s in enumerate(sizes):
        for j in range(s):
            a, b = (i + 1) % n, (i + 2) % n
            T.append((start[i] + j, start[a] + int(rng.integers(sizes[a])), start[b] + int(rng.integers(sizes[b]))))
    return permuted(V, np.array(T, i32), seed)


def one_cell():
    """More than two sort tiles of vertices in ONE cell: everything collapses, and the result is empty."""
    V, T = zigzag(2 * TILE + 100)
    return (V * f32(2.0 ** -12) + f32(0.25)).astype(f32), T


def duplicate_sets():
    """A strip no two vertices of which share a cell of 0.2, with copies of three of its triangles put in: a set of 2 whose copy is
    the FIRST triangle, a set of 3 that straddles the sort tile (indices 2047 and 2048), a set of 4 whose copies are the LAST
    triangles; windings mixed."""
    V, T = zigzag(2102)
    T = T.tolist()
    rot, rev = (lambda t: (t[1], t[2], t[0])), (lambda t: (t[0], t[2], t[1]))
    a, b, c = T[7], T[5], T[9]
    out = [rot(a)] + T[:TILE - 2] + [rev(b), rot(b)] + T[TILE - 2:] + [rev(c), rot(c), rev(rot(c))]
    assert out[TILE - 1] == rev(b) and out[TILE] == rot(b)
    return V, np.array(out, i32)


def sized(nv):
    """weld's strip of nv vertices with 40 twins, under a cell of 0.6: neighbours merge."""
    return WC.sized(nv)


def _case(mesh, cell, colors=False):
    V, T = mesh
    return V, T, (index_colors(len(V)) if colors else None), cell


SMALL = {
    "tetrahedron_apart": lambda: _case(tetrahedron(), 0.5),
    "torus_colored": lambda: _case(torus(), 0.75, colors=True),
    "fine_torus": lambda: _case(fine_torus(), 0.5, colors=True),
    "jittered_soup": lambda: _case(WC.jittered(), 0.1, colors=True),
    "flat_patch": lambda: _case(flat_patch(), 1.0),
    "crease": lambda: _case(crease(), 1.0, colors=True),
    "corner": lambda: _case(corner(), 0.75),
    "two_sheets": lambda: _case(two_sheets(), 1.0),
    "group_sizes": lambda: _case(group_sizes(), 1.0, colors=True),
    "thin_slab": lambda: _case(thin_slab(), 0.25),
    "nested_shells": lambda: _case(nested_shells(), 0.5),
    "corner_moved": lambda: _case((corner()[0] + MOVED, corner()[1]), 0.75),
    "torus_negative_faces": lambda: _case(fine_torus(), 0.25),
}
SIZES = (255, 256, 257, 2047, 2048, 2049)
WATERTIGHT = {
    "torus": lambda: (torus(), (0.75, 1.5)),
    "fine_torus": lambda: (fine_torus(), (0.25, 0.5, 1.0, 2.0)),
    "cube": lambda: (WC.cube(), (0.5, 2.0)),
    "corner": lambda: (corner(), (0.5, 0.75, 1.25)),
    "nested_shells": lambda: (nested_shells(), (0.5, 1.0)),
    "thin_slab": lambda: (thin_slab(), (0.25, 0.5)),
}


# ---- the recorded cases (the C++ suite) ------------------------------------------------------------------------------------------
RECORDED = ["tetrahedron_apart", "torus_colored", "jittered_soup", "crease", "two_sheets", "group_sizes", "thin_slab"]


def record(name):
    from tests import mesh_simplify_model as M
    V, T, cols, cell = SMALL[name]()
    out = {"mesh": name, "nv": len(V), "nt": len(T), "cell": float(f32(cell)), "colors": cols is not None, "runs": []}
    for placement in PLACEMENTS:
        for flags in FLAGS:
            s = M.simplify(V, T, cols, cell, placement, flags)
            out["runs"].append({"placement": placement, "flags": flags, "vertex_index": [int(x) for x in s.vertex_index],
                                "triangle_index": [int(x) for x in s.triangle_index], "triangles": [int(x) for x in s.triangles],
                                "vertices": [int(x) for x in s.vertices.view(u32).reshape(-1)],
                                "colors": [int(x) for x in s.colors.view(u32).reshape(-1)],
                                "stats": [int(s.merged), int(s.degenerate), int(s.duplicates), int(s.unreferenced), int(s.passes), int(s.fallbacks)]})
    return out


def load():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":
    if "--record" in sys.argv:
        with open(FIXTURE, "w") as f:
            json.dump({"cases": [record(n) for n in RECORDED]}, f, indent=None, separators=(",", ":"))
            f.write("\n")
        print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
