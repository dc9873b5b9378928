"""The meshes of the welding tests (tests/test_mesh_weld_host.py, tests/test_gpu_mesh_weld.py, tests/test_gpu_mesh_weld_cpp.py) and
the recorded results the C++ suite reads (tests/golden/mesh_weld_cases.json).  A case is (V (nv, 3) float32, T (nt, 3) int32,
colors (nv, 3) float32 or None, tolerance); coordinates are small decimals, so the positions are the same bits on every machine.

    python -m tests.mesh_weld_cases --record      rewrites the fixture from the model
"""
import json
import os
import sys

import numpy as np

from tests import mesh_topology_cases as TC
from tests.mesh_topology_cases import patch, permuted, tetrahedron, torus, with_degenerates, zigzag  # noqa: F401

f32, f64, i32, i64, u32 = np.float32, np.float64, np.int32, np.int64, np.uint32
ROOT = TC.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "mesh_weld_cases.json")
MOVED = np.array([4096, -8192, 1024], f32)
TINY = f32(2.0) ** -130
FLAGS = (0, 1, 2, 3)   # every combination of SDFK_WELD_KEEP_DEGENERATE (1) and SDFK_WELD_KEEP_UNREFERENCED (2)


def soup(V, T):
    """The mesh de-indexed: three vertices of its own per triangle."""
    T = np.asarray(T, i32).reshape(-1, 3)
    return np.ascontiguousarray(np.asarray(V, f32)[T.reshape(-1)]), np.arange(3 * len(T), dtype=i32).reshape(-1, 3)


def index_colors(nv):
    """A colour per INDEX (never zero): duplicates differ in colour, so the representative's must win."""
    k = np.arange(nv, dtype=f64)
    return np.stack([(k + 1) / 4096, ((k * 7) % 64 + 1) / 64, 1 - (k % 5) / 8], 1).astype(f32)


def cube():
    V = [(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)]
    T = [(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5)]
    return TC._mesh(V, T)


def with_duplicates(V, T, ndup, seed):
    """ndup copies of randomly chosen vertices appended; every corner that names a copied vertex goes to one of its copies with
    probability 1/2."""
    rng = np.random.default_rng(seed)
    V, T = np.asarray(V, f32), np.asarray(T, i32).copy()
    src = rng.integers(0, len(V), ndup)
    flat = T.reshape(-1)
    for k, s in enumerate(src):
        hit = np.flatnonzero((flat == s) & (rng.random(len(flat)) < 0.5))
        flat[hit] = len(V) + k
    return np.ascontiguousarray(np.concatenate([V, V[src]])), flat.reshape(-1, 3)


def one_coordinate_pairs():
    """Every vertex has a partner that differs from it in exactly one coordinate (which the first sort, or only the second, must
    keep apart) and an equal twin (which must weld): the boundary between the two sorts."""
    base = [(1, 2, 3), (1.5, 2, 3), (1, 2.5, 3), (1, 2, 3.5), (1, 2, 3), (1.5, 2, 3), (1, 2.5, 3), (1, 2, 3.5)]
    return TC._mesh(base, [(0, 1, 2), (4, 6, 7), (5, 3, 2), (1, 7, 4)])


def signed_zeros():
    """-0 against +0 in every coordinate: equal as values, so one group each."""
    z = f32(-0.0)
    V = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (z, z, z), (1, z, 0), (z, 1, z), (0, z, 1)], f32)
    return V, np.array([(0, 1, 2), (3, 4, 6), (5, 3, 6), (4, 5, 6)], i32)


def all_equal():
    return np.full((5, 3), 0.75, f32), np.array([(0, 1, 2), (2, 3, 4)], i32)


def first_and_last():
    """The first and the last index hold one position."""
    V, T = tetrahedron()
    return np.ascontiguousarray(np.concatenate([V, V[:1]])), np.concatenate([T[:2], np.array([(1, 2, 3), (4, 3, 2)], i32)])


def sized(nv, seed=0):
    """A strip with 40 duplicated vertices, nv vertices in all."""
    return with_duplicates(*zigzag(nv - 40), 40, seed=nv + seed)


def big_permuted_soup():
    """3 x 2049 vertices: the soup of a 2049-triangle strip, indices permuted -- the members of a group lie in different tiles."""
    return permuted(*soup(*zigzag(2051)), 6)


def unreferenced_and_degenerate():
    """with_degenerates (vertex 3 only in (2, 2, 3), vertex 4 only in (4, 4, 4)) plus a twin of vertex 1 that makes a triangle
    degenerate only after the weld, and a vertex nothing names."""
    V, T = with_degenerates()
    V = np.concatenate([V, V[1:2], np.array([(7, 7, 7)], f32)])
    return np.ascontiguousarray(V), np.concatenate([T, np.array([(1, 5, 2), (0, 5, 2)], i32)])


def jittered(tolerance=0.1, seed=2):
    """The soup of a patch whose vertices sit at cell centres of the lattice, every soup vertex jittered by less than a quarter
    of the tolerance per axis: the members of a group differ as values and share a cell."""
    V, T = patch(7, 5)
    rng = np.random.default_rng(seed)
    cell = np.stack([np.round(V[:, 0] / 0.5) - 3, np.round(V[:, 1] / 0.25) - 2, np.round(V[:, 2] / 0.125)], 1).astype(f64)
    S, ST = soup(cell, T)
    centre = (S.astype(f64) + 0.5) * f64(f32(tolerance))
    return (centre + rng.uniform(-0.24, 0.24, centre.shape) * f64(f32(tolerance))).astype(f32), ST


def straddling_pair():
    """Two vertices one ulp apart on the two sides of the cell face x = 0.5 of the lattice 0.25: they stay two."""
    below = np.nextafter(f32(0.5), f32(0))
    V = np.array([(0.5, 0.1, 0.1), (below, 0.1, 0.1), (0.9, 0.4, 0.1), (0.3, 0.4, 0.1)], f32)
    return V, np.array([(0, 2, 3), (1, 3, 2)], i32)


def _plain(mesh, colors=False, tolerance=0.0):
    V, T = mesh
    return V, T, (index_colors(len(V)) if colors else None), tolerance


SMALL = {
    "tetrahedron_soup": lambda: _plain(soup(*tetrahedron())),
    "cube_soup": lambda: _plain(soup(*cube())),
    "tetrahedron_clean": lambda: _plain(tetrahedron()),
    "one_coordinate_pairs": lambda: _plain(one_coordinate_pairs()),
    "signed_zeros": lambda: _plain(signed_zeros()),
    "all_equal": lambda: _plain(all_equal()),
    "first_and_last": lambda: _plain(first_and_last()),
    "unreferenced_and_degenerate": lambda: _plain(unreferenced_and_degenerate()),
    "torus_soup_colored": lambda: _plain(soup(*torus()), colors=True),
    "cube_soup_moved": lambda: _plain((soup(*cube())[0] + MOVED, soup(*cube())[1])),
    "strip_soup_tiny": lambda: _plain((soup(*zigzag(40))[0] * TINY, soup(*zigzag(40))[1])),
    "jittered_lattice": lambda: _plain(jittered(), colors=True, tolerance=0.1),
    "straddling_pair_lattice": lambda: _plain(straddling_pair(), tolerance=0.25),
    "cube_soup_lattice": lambda: _plain(soup(*cube()), tolerance=0.5),
}
SIZES = (255, 256, 257, 2047, 2048, 2049)


# ---- the recorded cases (the C++ suite) ------------------------------------------------------------------------------------------
RECORDED = list(SMALL)


def record(name):
    from tests import mesh_weld_model as M
    V, T, cols, tol = SMALL[name]()
    out = {"mesh": name, "nv": len(V), "nt": len(T), "tolerance": float(f32(tol)), "colors": cols is not None, "passes": M.passes(V, tol), "flags": []}
    for flags in FLAGS:
        w = M.weld(V, T, cols, tol, flags)
        out["flags"].append({"vertex_map": [int(x) for x in w.vertex_map], "vertex_index": [int(x) for x in w.vertex_index],
                             "triangle_index": [int(x) for x in w.triangle_index], "triangles": [int(x) for x in w.triangles],
                             "stats": [int(w.merged), int(w.degenerate), int(w.unreferenced)]})
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
