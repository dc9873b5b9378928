"""The meshes of the smoothing tests (tests/test_mesh_smooth_host.py, tests/test_gpu_mesh_smooth.py,
tests/test_gpu_mesh_smooth_cpp.py): the shapes of tests/mesh_topology_cases.py and three more, and the recorded results the C++
suite reads (tests/golden/mesh_smooth_cases.json).  Every mesh is (V (nv, 3) float32, T (nt, 3) int32).

    python -m tests.mesh_smooth_cases --record      rewrites the fixtures from the model
"""
import json
import os
import sys

import numpy as np

from tests import mesh_topology_cases as TC
from tests.mesh_topology_cases import (SMALL as TOPOLOGY_SMALL, fan, grid_permuted, no_area, patch, permuted, quad_strip, tetrahedron, torus,  # noqa: F401
                                       two_tetrahedra_out_of_order, vertex_colors, with_degenerates, zigzag)

f32, f64, i32, i64 = np.float32, np.float64, np.int32, np.int64
ROOT = TC.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "mesh_smooth_cases.json")
ACCURACY = os.path.join(ROOT, "tests", "golden", "mesh_smooth_accuracy.json")


def big_fan(n=300):
    """n triangles round vertex 0: its degree, n + 1, crosses a 256-lane block; an open fan, so the rim and the hub are boundary."""
    k = np.arange(n + 1)
    t = k.astype(f64) / f64(n)                                   # a quarter circle by its rational parametrisation: no libm
    ring = np.stack([(1 - t * t) / (1 + t * t), 2 * t / (1 + t * t), f64(0.001) * (k % 7)], 1)
    V = np.concatenate([np.zeros((1, 3)), ring]).astype(f32)
    T = np.stack([np.zeros(n, i64), 1 + np.arange(n), 2 + np.arange(n)], 1)
    return V, T.astype(i32)


def doubled_triangle():
    """One triangle listed twice: every neighbour appears once, and no edge is a boundary (each has two sides)."""
    return TC._mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0.5)], [(0, 1, 2), (0, 1, 2)])


def icosphere(subdivisions=3):
    """The unit icosphere: 642 vertices and 1280 triangles at 3 subdivisions, outward winding."""
    p = (1 + np.sqrt(f64(5))) / 2
    V = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, f64) / np.sqrt(f64(1) + p * p) for v in V]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = V[a] + V[b]
                V.append(m / np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]))
                mid[key] = len(V) - 1
            return mid[key]

        for a, b, c in T:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        T = out
    return np.array(V, f64).astype(f32), np.array(T, i32)


def noisy_icosphere(sigma=0.02, seed=1):
    V, T = icosphere()
    r = f64(1) + f64(sigma) * np.random.default_rng(seed).standard_normal(len(V))
    return (V.astype(f64) * r[:, None]).astype(f32), T


SMALL = dict(TOPOLOGY_SMALL)
SMALL.update({"big_fan_300": big_fan, "doubled_triangle": doubled_triangle, "noisy_icosphere": noisy_icosphere})

# the positions the host test also runs every small shape at
MOVED = np.array([4096, -8192, 1024], f32)
TINY, HUGE = f32(2.0) ** -130, f32(1e30)


def radii(P):
    r = np.sqrt((np.asarray(P, f64) ** 2).sum(axis=1))
    return float(r.std()), float(r.mean())


# ---- the recorded cases (the C++ suite) ------------------------------------------------------------------------------------------
RECORDED = ["tetrahedron", "patch_5x3", "torus_6x5", "fan", "two_tetrahedra_out_of_order", "with_degenerates", "no_area", "doubled_triangle"]
RECORDED_ITERATIONS, RECORDED_LAMBDA, RECORDED_MU = 3, 0.5, -0.53


def _bits(a):
    return [int(x) for x in np.ascontiguousarray(a, f32).view(np.uint32).reshape(-1)]


def record(name):
    from tests import mesh_smooth_model as M
    V, T = SMALL[name]()
    adj = M.adjacency(len(V), T)
    P = M.smooth(V, T, RECORDED_ITERATIONS, RECORDED_LAMBDA, RECORDED_MU, True, adj=adj)
    return {"mesh": name, "nv": len(V), "nt": len(T), "start": [int(x) for x in adj.start], "neighbors": [int(x) for x in adj.neighbors],
            "boundary": [int(x) for x in adj.boundary], "smoothed": _bits(P), "normals": _bits(M.vertex_normals(V, T)),
            "smoothed_normals_flipped": _bits(M.vertex_normals(P, T, flip=True))}


def accuracy():
    from tests import mesh_smooth_model as M
    V, T = noisy_icosphere()
    clean, _ = icosphere()
    taubin, laplace = M.smooth(V, T, 10, 0.5, -0.53, False), M.smooth(V, T, 10, 0.5, 0.0, False)
    N = M.vertex_normals(clean, T).astype(f64)
    unit = clean.astype(f64) / np.sqrt((clean.astype(f64) ** 2).sum(axis=1))[:, None]
    rows = {k: dict(zip(("std", "mean"), radii(P))) for k, P in (("noisy", V), ("taubin_10", taubin), ("laplacian_10", laplace))}
    rows["clean_normals_least_dot"] = float((N * unit).sum(axis=1).min())
    return rows


def load():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":
    if "--record" in sys.argv:
        with open(FIXTURE, "w") as f:
            json.dump({"iterations": RECORDED_ITERATIONS, "lambda": RECORDED_LAMBDA, "mu": RECORDED_MU, "cases": [record(n) for n in RECORDED]}, f,
                      indent=None, separators=(",", ":"))
            f.write("\n")
        with open(ACCURACY, "w") as f:
            json.dump(accuracy(), f, indent=1)
            f.write("\n")
        print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
