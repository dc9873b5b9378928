"""CPU check of mesh smoothing and vertex normals: sdfkit_amd/csrc/trimesh_adjacency.h (the functions the kernels of
lib_trimesh_smooth.hip call, built with g++ by tests/cpp/mesh_smooth_host.cpp and run one item at a time in the kernels' order)
against the numpy model (tests/mesh_smooth_model.py), bit for bit: the adjacency, the boundary bytes, the corners, smoothed
positions and normals of every small shape, also far from the origin, at subnormal and at huge scale.  Then the model itself: the
invariants of any adjacency, the boundary bytes of the hand-made shapes, and what smoothing does to a noisy sphere."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_smooth_cases as Cs
from tests import mesh_smooth_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, i32, i64, u32 = np.float32, np.float64, np.int32, np.int64, np.uint32

MESHES = dict(Cs.SMALL)
MESHES.update({"zigzag_257": lambda: Cs.zigzag(257), "patch_permuted": lambda: Cs.permuted(*Cs.patch(17, 9), 8),
               "strip_600_permuted": lambda: Cs.permuted(*Cs.quad_strip(600), 5)})

# (iterations, lambda, mu, pin, flip)
RUNS = [(0, 0.5, -0.53, True, False), (1, 0.5, 0.0, False, False), (2, 0.5, -0.53, True, True), (7, 0.33, -0.34, False, False)]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_smooth") / "mesh_smooth_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cpp", "mesh_smooth_host.cpp"), "-o", exe])
    return exe


def _run(exe, tmp_path, V, T, iterations, lam, mu, pin, flip):
    src, dst = str(tmp_path / "case.in"), str(tmp_path / "case.out")
    with open(src, "wb") as f:
        f.write(struct.pack("<4q2f", len(V), len(T), iterations, (1 if pin else 0) | (2 if flip else 0), lam, mu))
        f.write(np.ascontiguousarray(T, i32).tobytes() + np.ascontiguousarray(V, f32).tobytes())
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "mesh smooth ok" in p.stdout, (p.returncode, p.stderr)
    return np.fromfile(dst, u32)


def _compare(out, V, T, iterations, lam, mu, pin, flip, what):
    nv = len(V)
    adj, cor = M.adjacency(nv, T), M.corners(nv, T)
    top = (nv - 1).bit_length(), nv.bit_length()
    to_bytes, from_bytes = (top[0] + 7) // 8, (top[1] + 7) // 8
    assert out[0] == ((1 << to_bytes) - 1) | ((1 << from_bytes) - 1) << 4 and out[1] == (1 << from_bytes) - 1, what
    o = 2
    E = int(out[o]); o += 1
    assert E == len(adj.neighbors), what
    assert np.array_equal(out[o:o + nv + 1], adj.start), what; o += nv + 1
    assert np.array_equal(out[o:o + E], adj.neighbors), what; o += E
    assert np.array_equal(out[o:o + nv], adj.boundary), what; o += nv
    IE = int(out[o]); o += 1
    assert IE == len(cor.corners) == 3 * len(M.live(T)), what
    assert np.array_equal(out[o:o + nv + 1], cor.start), what; o += nv + 1
    assert np.array_equal(out[o:o + IE], cor.corners), what; o += IE
    P = M.smooth(V, T, iterations, lam, mu, pin, adj=adj)
    assert np.array_equal(out[o:o + 3 * nv], _bits(P).reshape(-1)), what; o += 3 * nv
    assert np.array_equal(out[o:o + 3 * nv], _bits(M.vertex_normals(V, T, cor=cor)).reshape(-1)), what; o += 3 * nv
    assert np.array_equal(out[o:o + 3 * nv], _bits(M.vertex_normals(P, T, flip=flip, cor=cor)).reshape(-1)), what; o += 3 * nv
    assert o == len(out), what
    return P


@pytest.mark.parametrize("name", list(MESHES))
def test_header_matches_model(host_exe, tmp_path, name):
    V, T = MESHES[name]()
    for run in RUNS:
        _compare(_run(host_exe, tmp_path, V, T, *run), V, T, *run, (name, run))


@pytest.mark.parametrize("name", list(Cs.SMALL))
def test_header_matches_model_far_tiny_and_huge(host_exe, tmp_path, name):
    """Moved to (4096, -8192, 1024): the means lose the low bits of the detail.  Scaled by 2^-130: every result is subnormal in
    float32.  Scaled by 1e30: the cross products reach 1e60 and their squares 1e120, inside binary64."""
    V, T = Cs.SMALL[name]()
    run = (2, 0.5, -0.53, True, False)
    with np.errstate(all="ignore"):
        for what, W in (("moved", V + Cs.MOVED), ("tiny", V * Cs.TINY), ("huge", V * Cs.HUGE)):
            P = _compare(_run(host_exe, tmp_path, W, T, *run), W, T, *run, (name, what))
            if what == "tiny":
                assert np.all(np.abs(P) < np.finfo(f32).tiny) and np.any(P != 0), name
                if name == "noisy_icosphere":
                    assert np.all(np.abs(np.sqrt((M.vertex_normals(P, T).astype(f64) ** 2).sum(axis=1)) - 1) < 1e-6)


def test_pinned_and_isolated_vertices_keep_their_bits(host_exe, tmp_path):
    """-0.0 coordinates on pinned vertices (the rim of a patch) and on isolated ones (an unreferenced vertex, the vertices of
    index-degenerate triangles only): copied as bits by every step."""
    V, T = Cs.patch(5, 3)
    V = np.concatenate([V, np.array([[-0.0, 3.0, -0.0]], f32)])
    rim = M.adjacency(len(V), T).boundary != 0
    V[rim, 2] = f32(-0.0)
    run = (3, 0.5, -0.53, True, False)
    P = _compare(_run(host_exe, tmp_path, V, T, *run), V, T, *run, "patch")
    assert np.array_equal(_bits(P[rim]), _bits(V[rim])) and np.array_equal(_bits(P[-1]), _bits(V[-1]))
    assert np.all(np.signbit(P[rim, 2])) and np.signbit(P[-1, 0]) and not np.array_equal(_bits(P[~rim][:-1]), _bits(V[~rim][:-1]))
    V, T = Cs.with_degenerates()
    V[3:] = np.array([[-0.0, 1.0, -0.0], [2.0, -0.0, 2.0]], f32)
    run = (2, 0.5, 0.0, False, False)
    P = _compare(_run(host_exe, tmp_path, V, T, *run), V, T, *run, "with_degenerates")
    assert np.array_equal(_bits(P[3:]), _bits(V[3:]))


# ---- the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_adjacency_invariants(name):
    V, T = MESHES[name]()
    nv = len(V)
    adj = M.adjacency(nv, T)
    sets = [set() for _ in range(nv)]
    for a, b, c in T[M.live(T)].tolist():
        sets[a] |= {b, c}; sets[b] |= {a, c}; sets[c] |= {a, b}
    start = adj.start.astype(i64)
    assert start[0] == 0 and start[-1] == len(adj.neighbors) and np.array_equal(start[1:] - start[:-1], adj.degree)
    for v in range(nv):
        row = adj.neighbors[start[v]:start[v + 1]].tolist()
        assert row == sorted(sets[v]) and v not in row, (name, v)          # ascending, each once, no self loop, the set-based degree
        assert all(v in adj.neighbors[start[w]:start[w + 1]] for w in row)   # symmetric
    cor = M.corners(nv, T)
    flat = np.asarray(T, i64).reshape(-1)
    cs = cor.start.astype(i64)
    for v in range(nv):
        row = cor.corners[cs[v]:cs[v + 1]].astype(i64)
        assert np.all(flat[row] == v) and np.all(np.diff(row) > 0), (name, v)
    assert len(cor.corners) == 3 * len(M.live(T))


def test_boundary_bytes_of_the_hand_made_shapes():
    V, T = Cs.patch(5, 3)
    b = M.adjacency(len(V), T).boundary.reshape(4, 6)
    rim = np.ones((4, 6), bool)
    rim[1:-1, 1:-1] = False
    assert np.array_equal(b != 0, rim) and int(b.sum()) == 2 * (5 + 3)      # exactly the perimeter
    for name in ("torus_6x5", "tetrahedron", "doubled_triangle"):
        V, T = Cs.SMALL[name]()
        assert not np.any(M.adjacency(len(V), T).boundary), name
    V, T = Cs.fan()
    once = {}
    for a, b_, c in T.tolist():
        for e in ((a, b_), (b_, c), (c, a)):
            once[frozenset(e)] = once.get(frozenset(e), 0) + 1
    assert once[frozenset((0, 1))] == 3
    on_once_used = {v for e, m in once.items() if m == 1 for v in e}
    assert np.array_equal(np.flatnonzero(M.adjacency(len(V), T).boundary).tolist(), sorted(on_once_used))
    V, T = Cs.doubled_triangle()
    assert M.adjacency(3, T).neighbors.tolist() == [1, 2, 0, 2, 0, 1]
    V, T = Cs.big_fan()
    assert int(M.adjacency(len(V), T).degree[0]) == 301


def test_smoothing_a_noisy_sphere():
    """Inequalities between model runs (the numbers themselves are recorded in tests/golden/mesh_smooth_accuracy.json for the
    reader: std of |v| 0.0191 -> 0.0073 (Taubin) / 0.0043 (Laplacian); mean of |v| 0.9995 -> 1.0024 / 0.9443)."""
    V, T = Cs.noisy_icosphere()
    assert len(V) == 642 and len(T) == 1280
    taubin, laplace = M.smooth(V, T, 10, 0.5, -0.53, False), M.smooth(V, T, 10, 0.5, 0.0, False)
    (s0, m0), (st, mt), (sl, ml) = Cs.radii(V), Cs.radii(taubin), Cs.radii(laplace)
    print("std, mean of |v|: noisy", s0, m0, "taubin", st, mt, "laplacian", sl, ml)
    assert st < s0 and sl < s0
    assert abs(mt - m0) < abs(ml - m0)
    with open(Cs.ACCURACY) as f:
        rec = json.load(f)
    assert set(rec) == {"noisy", "taubin_10", "laplacian_10", "clean_normals_least_dot"}


def test_normals_of_the_clean_sphere_point_outward():
    V, T = Cs.icosphere()
    N = M.vertex_normals(V, T).astype(f64)
    unit = V.astype(f64) / np.sqrt((V.astype(f64) ** 2).sum(axis=1))[:, None]
    dots = (N * unit).sum(axis=1)
    print("least dot", dots.min())
    assert np.all(dots > 0)
    assert np.all(M.vertex_normals(V, T, flip=True).astype(f64) == -N)
    V, T = Cs.no_area()
    assert not np.any(_bits(M.vertex_normals(V, T)))       # (+0, +0, +0), also flipped
    assert not np.any(_bits(M.vertex_normals(V, T, flip=True)))


def test_marching_cubes_meshes_wind_with_their_gradient_normals():
    """On the golden marching-cubes meshes (b - a) x (c - a) points the way the gradient normals do, at every vertex: the
    unflipped vertex normals are the ones a mesh of this project wants."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "small_meshes.npz"))
    for name in ("Sphere10", "CreateMeshSphere"):
        V, T, present = z[name + ".vertices"], z[name + ".triangles"], z[name + ".normals"]
        pos, neg = M.side_votes(M.vertex_normals(V, T), present)
        assert (pos, neg) == (len(V), 0), name


def test_recorded_cases_are_what_the_model_gives_today():
    doc = Cs.load()
    assert [c["mesh"] for c in doc["cases"]] == Cs.RECORDED
    assert doc["cases"] == [Cs.record(n) for n in Cs.RECORDED]
    assert (doc["iterations"], doc["lambda"], doc["mu"]) == (Cs.RECORDED_ITERATIONS, Cs.RECORDED_LAMBDA, Cs.RECORDED_MU)
    assert os.path.getsize(Cs.FIXTURE) < 64 << 10
