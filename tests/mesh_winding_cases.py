"""The cases of the winding-number tests (tests/test_mesh_winding_host.py on the CPU, tests/test_gpu_mesh_winding.py on the device):
small meshes -- closed, inside out, open, overlapping, nested, degenerate -- with the queries at which the sum of
csrc/trimesh_winding.h can still go wrong.  A case is a dict: V (nv, 3) f32, T (nt, 3) int32, Q (n, 3) f32 point queries, and a
volume: mn, mx, n = (nx, ny, nz global), z0, nz (local planes), band.  Everything is deterministic; the marching-cubes spheres come
from the CPU reference (oracle), whose meshes the library reproduces bit for bit, and are made once."""
import functools
import json
import os

import numpy as np

from tests import mesh_ray_cases as RC
from tests import mesh_winding_model as M
from tests import meshsdf_model as MM

f32, f64, i32 = np.float32, np.float64, np.int32
INF = np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "tests", "golden", "mesh_winding_accuracy.json")
BETAS = (1.5, 2.0, 2.5, 3.0, 4.0)          # the recorded list; DEFAULT_BETA is chosen from it (see the JSON's "default")
DEFAULT_BETA = 2.5                         # sdfkit_amd.meshsdf.DEFAULT_WINDING_BETA repeats it


def flipped(T):
    return np.ascontiguousarray(np.asarray(T, i32).reshape(-1, 3)[:, ::-1])


def concat(*meshes):
    Vs, Ts, base = [], [], 0
    for V, T in meshes:
        V, T = np.asarray(V, f32).reshape(-1, 3), np.asarray(T, i32).reshape(-1, 3)
        Vs.append(V)
        Ts.append(T + base)
        base += len(V)
    return np.concatenate(Vs), np.concatenate(Ts)


def feature_points(V, T):
    """every vertex, edge midpoint and face centre (f32)"""
    V, T = np.asarray(V, f32).reshape(-1, 3), np.asarray(T, np.int64).reshape(-1, 3)
    e = RC.edges_of(T)
    mid = ((V[e[:, 0]].astype(f64) + V[e[:, 1]]) / 2).astype(f32)
    face = ((V[T[:, 0]].astype(f64) + V[T[:, 1]] + V[T[:, 2]]) / 3).astype(f32)
    return np.concatenate([V[np.unique(T)], mid, face])


def scattered(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (n, 3)).astype(f32)


def far_points(centre, seed, n=24):
    d = RC.directions(n, seed).astype(f64)
    r = np.repeat([50.0, 1e3, 1e6, 1e12], n // 4)[:, None]
    return (np.asarray(centre, f64) + d * r).astype(f32)


def lattice_faces(V, T, seed, n=96):
    """queries on the faces of the hierarchy's lattice: one coordinate on a cell face, the others anywhere in the box"""
    H = M.build(V, T)
    rng = np.random.default_rng(seed)
    lo = H.lo.astype(f64)
    cells = 1 << H.L
    q = lo + rng.uniform(0, cells, (n, 3)) / H.scale
    ax = rng.integers(0, 3, n)
    q[np.arange(n), ax] = lo[ax] + rng.integers(0, cells + 1, n) / H.scale
    return q.astype(f32)


def _case(V, T, Q, mn, mx, n, z0=0, nz=None, band=INF, closed=False):
    V = np.ascontiguousarray(np.asarray(V, f32).reshape(-1, 3))
    T = np.ascontiguousarray(np.asarray(T, i32).reshape(-1, 3))
    Q = np.ascontiguousarray(np.asarray(Q, f32).reshape(-1, 3))
    return {"V": V, "T": T, "Q": Q, "mn": [float(x) for x in mn], "mx": [float(x) for x in mx], "n": tuple(n), "z0": z0,
            "nz": n[2] - z0 if nz is None else nz, "band": float(band), "closed": closed}


def _std_queries(V, T, lo, hi, seed, n=160):
    c = (np.asarray(lo, f64) + np.asarray(hi, f64)) / 2
    return np.concatenate([feature_points(V, T), scattered(n, lo, hi, seed), far_points(c, seed + 1)])


CUBE = MM.box_mesh([0, 0, 0], [1, 1, 1])
OCTA = MM.octahedron([0.25, -0.5, 0.125], 1.0)


def cube():
    V, T = CUBE
    return _case(V, T, _std_queries(V, T, [-0.5] * 3, [1.5] * 3, 1), [-0.55, -0.5, -0.45], [1.5, 1.55, 1.6], (11, 13, 21), closed=True)


def octahedron():
    V, T = OCTA
    return _case(V, T, _std_queries(V, T, [-1, -1.75, -1.125], [1.5, 0.75, 1.375], 2), [-1.05, -1.8, -1.2], [1.6, 0.8, 1.4], (14, 12, 17), closed=True)


def cube_inside_out():
    c = cube()
    c["T"] = flipped(c["T"])
    return c


def octahedron_inside_out():
    c = octahedron()
    c["T"] = flipped(c["T"])
    return c


def cube_no_lid():
    V, T = CUBE
    T = np.asarray(T, i32).reshape(-1, 3)
    T = np.delete(T, [2, 3], 0)            # the two triangles of the z = 1 face
    return _case(V, T, _std_queries(V, T, [-0.5] * 3, [1.5] * 3, 3), [-0.55, -0.5, -0.45], [1.5, 1.55, 1.6], (12, 12, 19))


def _sphere_without(n, keep):
    V, T = RC.mc_sphere(n)
    ctr = (V[T[:, 0]].astype(f64) + V[T[:, 1]] + V[T[:, 2]]) / 3
    return V, np.ascontiguousarray(T[keep(ctr)])


def hemisphere():
    V, T = _sphere_without(16, lambda c: c[:, 2] < 0.0)
    return _case(V, T, np.concatenate([scattered(200, [-1.2] * 3, [1.2] * 3, 4), far_points([0, 0, 0], 5)]), [-1.25] * 3, [1.25] * 3, (16, 16, 20))


CAP_Z = 0.75          # the capped-off sphere: triangles whose centroid lies above this z are removed (radius 1)


def sphere_cap_removed():
    V, T = _sphere_without(24, lambda c: c[:, 2] < CAP_Z)
    Q = np.concatenate([scattered(200, [-1.2] * 3, [1.2] * 3, 6), lattice_faces(V, T, 7), far_points([0, 0, 0], 8)])
    return _case(V, T, Q, [-1.25] * 3, [1.25] * 3, (20, 20, 23))


TWO_A, TWO_B = ([0, 0, 0], [1, 1, 1]), ([0.5, 0.375, 0.25], [1.5, 1.375, 1.25])


def two_cubes():
    V, T = concat(MM.box_mesh(*TWO_A), MM.box_mesh(*TWO_B))
    return _case(V, T, _std_queries(V, T, [-0.5] * 3, [2.0] * 3, 9), [-0.5, -0.45, -0.41], [2.0, 1.9, 1.8], (20, 18, 22))


def nested_shells():
    Vo, To = MM.box_mesh([0, 0, 0], [3, 3, 3])
    Vi, Ti = MM.box_mesh([1, 1, 1], [2, 2, 2])
    V, T = concat((Vo, To), (Vi, flipped(Ti)))       # the inner shell faces into the cavity
    return _case(V, T, _std_queries(V, T, [-0.5] * 3, [3.5] * 3, 10), [-0.5, -0.4, -0.6], [3.5, 3.6, 3.4], (16, 17, 18), closed=True)


def degenerate():
    """an octahedron with every triangle twice, plus triangles of zero area: two equal vertices, three collinear ones, a point"""
    V, T = OCTA
    T = np.asarray(T, i32).reshape(-1, 3)
    extra = np.array([[0, 0, 2], [0, 1, 1], [3, 3, 3]], i32)
    Vx = np.concatenate([V, np.array([[0.25, -0.5, 3.0], [0.25, -0.5, 4.0], [0.25, -0.5, 5.0]], f32)])
    line = np.array([[6, 7, 8]], i32)
    T2 = np.concatenate([T, extra, T, line])
    Q = np.concatenate([_std_queries(V, T, [-1, -1.75, -1.125], [1.5, 0.75, 1.375], 11), np.array([[0.25, -0.5, 3.5], [0.25, -0.5, 4.0], [0.3, -0.5, 3.5]], f32)])
    return _case(Vx, T2, Q, [-1.05, -1.8, -1.2], [1.6, 0.8, 1.4], (10, 10, 10))


def big_sphere():
    """L >= 2: near queries open every level, far ones stop at the root"""
    V, T = RC.mc_sphere(32)
    Q = np.concatenate([scattered(256, [-1.2] * 3, [1.2] * 3, 12), lattice_faces(V, T, 13), far_points([0, 0, 0], 14),
                        feature_points(V, T)[::97]])
    return _case(V, T, Q, [-1.25] * 3, [1.25] * 3, (16, 16, 24), z0=8, nz=9, band=0.2, closed=True)


def _count(n):
    V, T = concat(MM.box_mesh(*TWO_A), MM.box_mesh(*TWO_B))
    return _case(V, T, scattered(n, [-0.5] * 3, [2.0] * 3, 20 + n), [-0.5] * 3, [2.0] * 3, (4, 4, 5))


def bad_queries():
    V, T = CUBE
    Q = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [0.5, 0.5, 0.5], [np.inf, np.inf, np.inf],
                  [3e38, 0.5, 0.5], [2.0, 2.0, 2.0]], f32)
    return _case(V, T, Q, [-0.5] * 3, [1.5] * 3, (4, 4, 5))


def banded_cube():
    V, T = CUBE
    return _case(V, T, scattered(32, [-0.5] * 3, [1.5] * 3, 30), [-0.55, -0.5, -0.45], [1.5, 1.55, 1.6], (11, 13, 21), band=0.15, closed=True)


CASES = {
    "cube": cube, "octahedron": octahedron, "cube_inside_out": cube_inside_out, "octahedron_inside_out": octahedron_inside_out,
    "cube_no_lid": cube_no_lid, "hemisphere": hemisphere, "sphere_cap_removed": sphere_cap_removed, "two_cubes": two_cubes,
    "nested_shells": nested_shells, "degenerate": degenerate, "big_sphere": big_sphere, "banded_cube": banded_cube,
    "count_255": lambda: _count(255), "count_256": lambda: _count(256), "count_257": lambda: _count(257), "bad_queries": bad_queries,
}
CLOSED = ("cube", "octahedron", "cube_inside_out", "octahedron_inside_out", "nested_shells", "big_sphere", "banded_cube")
OPEN = ("cube_no_lid", "hemisphere", "sphere_cap_removed")
# the cases of the accuracy table: their volumes' cell centres are the queries
RECORDED = ("cube", "octahedron", "cube_inside_out", "cube_no_lid", "hemisphere", "sphere_cap_removed", "two_cubes", "nested_shells",
            "big_sphere")


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    for k in ("V", "T", "Q"):
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def tree(name):
    c = case(name)
    return M.build(c["V"], c["T"])


@functools.lru_cache(maxsize=None)
def model(name, beta=DEFAULT_BETA):
    """the model's answer for the point queries"""
    return M.winding(tree(name), case(name)["Q"], beta)


def voxel_centres(c):
    return M.centres(c["mn"], c["mx"], c["n"], c["z0"], c["nz"])


@functools.lru_cache(maxsize=None)
def volume_model(name, beta=DEFAULT_BETA):
    """the model's answer at the cell centres of the case's volume (z fastest)"""
    return M.winding(tree(name), voxel_centres(case(name)), beta)


@functools.lru_cache(maxsize=None)
def volume_brute(name):
    c = case(name)
    return M.brute(c["V"], c["T"], voxel_centres(c))


def measure(name, beta):
    """(max |w_model - w_brute| over the volume's voxels, the share of voxels whose brute |w| lies within that of 1/2)"""
    wb = volume_brute(name)
    err = float(np.abs(volume_model(name, beta).w - wb).max())
    return err, float((np.abs(np.abs(wb) - 0.5) <= err).mean())


def recorded():
    with open(ACCURACY) as f:
        return json.load(f)


def record():
    """Writes tests/golden/mesh_winding_accuracy.json from the model (run by hand when the cases or the statement change):
    python -c "from tests import mesh_winding_cases as C; C.record()" """
    out = {"betas": list(BETAS), "default": DEFAULT_BETA, "cases": {}}
    for name in RECORDED:
        rows = {}
        for beta in BETAS:
            err, share = measure(name, beta)
            wb = volume_brute(name)
            flips = int((volume_model(name, beta).inside != (np.abs(wb) > 0.5)).sum())
            rows[repr(beta)] = {"max_error": err, "margin_share": share, "sign_flips": flips}
        out["cases"][name] = rows
    with open(ACCURACY, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


# ---- the host program (tests/cpp/mesh_winding_host.cpp): the header's walk on the CPU --------------------------------------------
def build_host(directory, sanitize=False):
    import subprocess
    exe = os.path.join(str(directory), "mesh_winding_host" + ("_san" if sanitize else ""))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall"] + extra +
                          [os.path.join(ROOT, "tests", "cpp", "mesh_winding_host.cpp"), "-o", exe])
    return exe


class HostResult:
    pass


def host_run(exe, directory, V, T, Q, beta, tag="w"):
    import struct
    import subprocess
    Q = np.ascontiguousarray(np.asarray(Q, f32).reshape(-1, 3))
    src, dst = os.path.join(str(directory), f"{tag}.in"), os.path.join(str(directory), f"{tag}.out")
    with open(src, "wb") as f:
        f.write(struct.pack("<3q2f", len(V), len(T), len(Q), beta, 0.0) + V.tobytes() + T.tobytes() + Q.tobytes())
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "mesh winding ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    out = np.fromfile(dst, np.int64)
    R = HostResult()
    R.L, R.occupied, R.max_leaf, R.cluster_terms, R.triangle_terms, R.differs, n, total = (int(x) for x in out[:8])
    rows = out[8:8 + 4 * n].reshape(n, 4)
    R.w = np.ascontiguousarray(rows[:, 0]).view(f64)
    R.inside = rows[:, 1].astype(bool)
    R.clusters, R.triangles = rows[:, 2], rows[:, 3]
    nodes = out[8 + 4 * n:].reshape(total, 9)
    R.count, R.start = nodes[:, 0], nodes[:, 1]
    R.N, R.P, R.r2 = np.ascontiguousarray(nodes[:, 2:5]).view(f64), np.ascontiguousarray(nodes[:, 5:8]).view(f64), np.ascontiguousarray(nodes[:, 8]).view(f64)
    return R
