"""The meshes of the topology tests (tests/test_mesh_topology_host.py, tests/test_gpu_mesh_topology.py,
tests/test_gpu_mesh_topology_cpp.py) and the recorded rows the C++ suite reads (tests/golden/mesh_topology_cases.json).  Every
mesh is (V (nv, 3) float32, T (nt, 3) int32); coordinates are small decimals and products of them in float32, so the positions
(and with them the area weights) are the same bits on every machine.

    python -m tests.mesh_topology_cases --record      rewrites the fixture from the model
"""
import json
import os
import sys

import numpy as np

f32, i32 = np.float32, np.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mesh_topology_cases.json")

_TET_V = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
_TET_T = [(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)]   # outward, every edge once each way


def _mesh(V, T):
    return np.array(V, f32).reshape(-1, 3), np.array(T, i32).reshape(-1, 3)


def tetrahedron():
    return _mesh(_TET_V, _TET_T)


def tetrahedron_reversed():
    V, T = tetrahedron()
    T[2] = T[2][::-1]
    return V, T


def bow_tie():
    """Two tetrahedra that share vertex 0: one component (connectivity is by index)."""
    second = {0: 0, 1: 4, 2: 5, 3: 6}
    V = _TET_V + [(-1, 0, 0), (0, -1, 0), (0, 0, -1)]
    return _mesh(V, _TET_T + [tuple(second[i] for i in t) for t in _TET_T])


def patch(qx, qy):
    """An open patch of qx x qy quads, two triangles each, consistently wound."""
    V = [(0.5 * i, 0.25 * j, 0.125 * ((i * j) % 3)) for j in range(qy + 1) for i in range(qx + 1)]
    T = []
    for j in range(qy):
        for i in range(qx):
            a = j * (qx + 1) + i
            b, c, d = a + 1, a + qx + 1, a + qx + 2
            T += [(a, b, d), (a, d, c)]
    return _mesh(V, T)


def torus(n=6, m=5):
    ring = [(2, 0), (1, 2), (-1, 2), (-2, 0), (-1, -2), (1, -2), (3, 1), (3, -1)][:n]
    tube = [(1, 0), (0.5, 1), (-0.5, 0.5), (-0.5, -0.5), (0.5, -1), (1, -0.5)][:m]
    V = [(f32(cx) * (f32(1) + f32(0.25) * f32(r)), f32(cy) * (f32(1) + f32(0.25) * f32(r)), f32(0.5) * f32(z)) for cx, cy in ring for r, z in tube]
    T = []
    for i in range(n):
        for j in range(m):
            a, b = i * m + j, i * m + (j + 1) % m
            c, d = ((i + 1) % n) * m + j, ((i + 1) % n) * m + (j + 1) % m
            T += [(a, c, d), (a, d, b)]
    return _mesh(V, T)


def moebius(n=8):
    """n quads in a ring, the last joined to the first with a half twist."""
    V = [(0.5 * i, j, 0.25 * ((i * (i + j)) % 4)) for i in range(n) for j in range(2)]
    T = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        c, d = (2 * (i + 1), 2 * (i + 1) + 1) if i + 1 < n else (1, 0)
        T += [(a, c, d), (a, d, b)]
    return _mesh(V, T)


def fan():
    """Three triangles on the edge (0, 1)."""
    return _mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0.5), (0, 0, 1)], [(0, 1, 2), (0, 1, 3), (0, 1, 4)])


def two_tetrahedra_out_of_order():
    """The tetrahedron of vertices 5 .. 8 is listed first; vertex 4 is referenced by nothing: numbering goes by root."""
    V = _TET_V + [(9, 9, 9)] + [(x + 3, y, z) for x, y, z in _TET_V]
    return _mesh(V, [tuple(i + 5 for i in t) for t in _TET_T] + _TET_T)


def with_degenerates():
    return _mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (2, 2, 2)], [(0, 1, 2), (2, 2, 3), (4, 4, 4)])


def no_area():
    """Two components, every triangle collinear: the area weights are all zero and nothing is refused."""
    return _mesh([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0)], [(0, 1, 2), (3, 4, 5)])


SMALL = {"tetrahedron": tetrahedron, "tetrahedron_reversed": tetrahedron_reversed, "bow_tie": bow_tie, "patch_5x3": lambda: patch(5, 3),
         "torus_6x5": torus, "moebius_8": moebius, "fan": fan, "two_tetrahedra_out_of_order": two_tetrahedra_out_of_order,
         "with_degenerates": with_degenerates, "no_area": no_area}

# F, V, E, boundary, non-manifold, odd, inconsistent of the single component (the issue's table)
EXPECTED = {"tetrahedron": (4, 4, 6, 0, 0, 0, 0), "tetrahedron_reversed": (4, 4, 6, 0, 0, 0, 3), "bow_tie": (8, 7, 12, 0, 0, 0, 0),
            "patch_5x3": (30, 24, 53, 16, 0, 16, 0), "torus_6x5": (60, 30, 90, 0, 0, 0, 0), "moebius_8": (16, 16, 32, 16, 0, 16, 1),
            "fan": (3, 5, 7, 6, 1, 7, 0)}


# ---- the sizes that straddle the machinery ---------------------------------------------------------------------------------------
def zigzag(nv):
    """A triangle strip over nv vertices: nv - 2 triangles, consistently wound, one component."""
    V = [(0.25 * (i // 2), i % 2, 0.125 * (i % 5)) for i in range(nv)]
    T = [(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(nv - 2)]
    return _mesh(V, T)


def quad_strip(nq):
    """nq quads in a row: 2 (nq + 1) vertices in order along the strip, 2 nq triangles.  The deep-tree case of the label rounds."""
    i = np.arange(nq + 1)
    V = np.zeros((2 * (nq + 1), 3), f32)
    V[0::2, 0] = V[1::2, 0] = (i % 1024).astype(f32) * f32(0.5)
    V[1::2, 1] = 1
    V[:, 2] = np.repeat((i // 1024).astype(f32), 2)
    a = 2 * np.arange(nq)
    T = np.stack([np.stack([a, a + 2, a + 3], 1), np.stack([a, a + 3, a + 1], 1)], 1).reshape(-1, 3)
    return V, T.astype(i32)


def permuted(V, T, seed):
    """The same mesh with its vertex indices permuted and its triangles shuffled."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(V))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(V))
    return np.ascontiguousarray(V[perm]), np.ascontiguousarray(inv[T][rng.permutation(len(T))].astype(i32))


def grid_permuted(n=300, seed=11):
    V, T = patch(n - 1, n - 1)
    return permuted(V, T, seed)


def tetrahedra(count=300, seed=3):
    """`count` disjoint tetrahedra of growing size, vertex indices permuted, triangle order shuffled."""
    V = np.concatenate([(np.array(_TET_V, f32) * f32(1 + (k % 7)) + np.array([3 * (k % 20), 3 * (k // 20), 0], f32)) for k in range(count)])
    T = np.concatenate([np.array(_TET_T, i32) + 4 * k for k in range(count)])
    return permuted(V.astype(f32), T, seed)


def vertex_colors(V):
    V = np.asarray(V, f32).reshape(-1, 3)
    return np.ascontiguousarray(np.stack([(V[:, 0] * f32(0.25)) % f32(1), (V[:, 1] * f32(0.5)) % f32(1), f32(1) - (V[:, 2] * f32(0.125)) % f32(1)], 1).astype(f32))


# ---- the recorded cases (the C++ suite) ------------------------------------------------------------------------------------------
RECORDED = list(SMALL)


def keep_pattern(count):
    """The select case recorded with every mesh: the even-numbered components."""
    return [c % 2 == 0 for c in range(count)]


def record(name):
    from tests import mesh_topology_model as M
    V, T = SMALL[name]()
    t = M.topology(V, T)
    s = M.select(V, T, keep_pattern(t.count), topo=t)
    return {"mesh": name, "nv": len(V), "nt": len(T), "census": [int(x) for x in t.census], "rows": [[int(x) for x in r] for r in t.rows],
            "vertex": [int(x) for x in t.vertex], "triangle": [int(x) for x in t.triangle],
            "select": {"vertex_index": [int(x) for x in s.vertex_index], "triangle_index": [int(x) for x in s.triangle_index],
                       "triangles": [int(x) for x in s.triangles]}}


def load():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":
    if "--record" in sys.argv:
        with open(FIXTURE, "w") as f:
            json.dump({"cases": [record(n) for n in RECORDED]}, f, indent=None, separators=(",", ":"))
            f.write("\n")
        print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
