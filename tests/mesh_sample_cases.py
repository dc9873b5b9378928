"""The meshes of the mesh-sampling tests (tests/test_gpu_mesh_sample.py, tests/test_gpu_mesh_sample_cpp.py,
tests/test_mesh_sample_host.py), the smallest at which each part of sdfk_trimesh_sample can go wrong, and the recorded cases of
tests/golden/mesh_sample_cases.json:

    python -m tests.mesh_sample_cases            writes the "cases" of the fixture from the numpy model (tests/mesh_sample_model.py)

The fixture's "icp" entry is recorded by tests/test_gpu_mesh_sample.py::test_end_to_end_registration (it needs the device's mesh
and registration); this script keeps it as it is."""
import json
import os

import numpy as np

from tests import mesh_sample_model as S
from tests import meshsdf_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mesh_sample_cases.json")
f32, f64 = np.float32, np.float64

UNIT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f64)


def _soup(tris):
    V = np.concatenate(tris).astype(f32)
    return V, np.arange(len(V), dtype=np.int32)


def one_triangle():
    return _soup([np.array([[0.25, -1, 0.5], [2, 0.5, -0.75], [-0.5, 1.5, 1]])])


def weight_quantisation():
    """A unit right triangle, copies scaled by 2^-16 (weight exactly 1) and 2^-17 (weight exactly 0) -- every coordinate exact in
    f32 --, and zero-area triangles first, last and in between."""
    return _soup([UNIT * 0, UNIT * 2.0 ** -17, UNIT, UNIT * 2.0 ** -16 + 3, UNIT[[0, 1, 1]], UNIT * 2.0 ** -17 - 2, UNIT * 2.0 ** -16 - 5,
                  UNIT[[2, 2, 2]]])


def degenerate_interleaved(seed=3):
    """40 triangles: every even one (the first included) and the last one without area -- a point, two coincident vertices or
    three collinear ones -- between random real ones."""
    rng = np.random.default_rng(seed)
    tris = []
    for i in range(40):
        t = rng.uniform(-1, 1, (3, 3))
        if i % 2 == 0 or i == 39:
            t = np.round(t * 32) / 32      # (on a lattice: the collinear ones are exactly collinear in f32)
            t = [t[[0, 0, 0]], t[[0, 1, 1]], np.stack([t[0], t[0] + (t[1] - t[0]) * 0.5, t[1]])][i % 3]
        tris.append(t)
    return _soup(tris)


def all_degenerate():
    return _soup([UNIT * 0 + 2, UNIT[[0, 1, 1]], np.array([[0, 0, 0], [1, 1, 1], [3, 3, 3]], f64)])


def sheet(nx=50, ny=50, seed=4):
    """A 50 x 50 x 1 sheet of quads with jittered vertices: 5000 triangles, more than two blocks of the scan."""
    rng = np.random.default_rng(seed)
    X, Y = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    V = np.stack([X, Y, np.zeros_like(X)], -1).reshape(-1, 3).astype(f64) + rng.uniform(-0.3, 0.3, ((nx + 1) * (ny + 1), 3))
    i = (X[:-1, :-1] * (ny + 1) + Y[:-1, :-1]).reshape(-1)
    T = np.stack([i, i + ny + 1, i + ny + 2, i, i + ny + 2, i + 1], 1).reshape(-1)
    return (V * 0.04).astype(f32), T.astype(np.int32)


def box():
    return MM.box_mesh([-0.5, -1.0, -0.25], [1.5, 1.0, 0.75])


def vertex_colors(V):
    """A colour per vertex that varies over the mesh (a function of the position, exact in f32 arithmetic or not: it is an input)."""
    V = np.asarray(V, f64)
    c = np.stack([0.5 + 0.25 * np.sin(3 * V[:, 0]), 0.5 + 0.25 * np.cos(2 * V[:, 1]), 0.25 + 0.125 * (V[:, 2] - np.floor(V[:, 2]))], 1)
    return c.astype(f32)


# ---- the recorded cases -----------------------------------------------------------------------------------------------------
RECORDED = [("box", box, 1000, 7, True), ("box", box, 1000, 7, False), ("weight_quantisation", weight_quantisation, 4099, 2 ** 64 - 1, True),
            ("sheet", sheet, 100003, 0, True), ("sheet", sheet, 3, 5, True)]
FIRST = 32


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def output_bytes(R):
    """Points, Normals, Colors, Triangles, Weights of a sampling result, concatenated."""
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (R.Points, R.Normals, R.Colors, R.Triangles, R.Weights))


def record(name, make, n, seed, stratified):
    V, T = make()
    R = S.sample(V, T, n, seed, stratified, colors=vertex_colors(V))
    k = min(n, FIRST)
    nz, total = S.stats(V, T)
    return {"mesh": name, "n": n, "seed": seed, "stratified": stratified, "stats": [nz, total], "hash": f"{fnv1a64(output_bytes(R)):016x}",
            "triangles": R.Triangles[:k].tolist(),
            **{key: np.ascontiguousarray(a[:k], f32).view(np.uint32).reshape(-1).tolist()
               for key, a in (("points", R.Points), ("normals", R.Normals), ("colors", R.Colors), ("weights", R.Weights))}}


def load():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":
    old = load() if os.path.exists(FIXTURE) else {}
    doc = {"cases": [record(*c) for c in RECORDED], "icp": old.get("icp")}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
