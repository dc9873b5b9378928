"""CPU check of the mesh-sampling arithmetic (sdfkit_amd/csrc/trimesh_sample.h, the functions the kernels call, built with
g++ -ffp-contract=off by tests/cpp/mesh_sample_host.cpp) against the numpy model (tests/mesh_sample_model.py), bit for bit: the
normal and area term, the integer weight, the draws, the pick in both modes, the search of the prefix sums, the fold at its edge
cases, the point, the normal and the f32 weights.  Then invariants of the model alone on recorded meshes
(tests/golden/small_meshes.npz)."""
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_sample_cases as Cs
from tests import mesh_sample_model as S
from tests import meshsdf_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, u64 = np.float32, np.float64, np.uint64
SMALL = np.load(os.path.join(ROOT, "tests", "golden", "small_meshes.npz"))
ONE53 = 1 << 53


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_sample") / "mesh_sample_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "mesh_sample_host.cpp"),
                           "-o", exe])
    return exe


def _run(exe, mode, data, tmp_path, out_dtype):
    src, dst = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
    np.ascontiguousarray(data).tofile(src)
    p = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "mesh sample ok" in p.stdout, p.stderr
    return np.fromfile(dst, out_dtype)


def _triangles(rng):
    """(n, 3, 3) float32: random, needles, collinear, coincident vertices, points, coordinates of 1e6, subnormal coordinates."""
    tris = [rng.uniform(-2, 2, (400, 3, 3))]
    base = rng.uniform(-1, 1, (60, 3))
    d = rng.uniform(-1, 1, (60, 3))
    tris.append(np.stack([base, base + d, base + d * 1e-6 + rng.uniform(-1e-7, 1e-7, (60, 3))], 1))   # needles
    tris.append(np.stack([base, base + d, base + 2 * d], 1))                                        # collinear
    tris.append(np.stack([base, base, base + d], 1))                                                # coincident vertices
    tris.append(np.stack([base, base, base], 1))                                                    # a point
    tris.append(rng.uniform(-1, 1, (40, 3, 3)) * 1e6)
    T = np.concatenate(tris).astype(f32)
    sub = (rng.integers(-2000, 2000, (40, 3, 3)).astype(f64) * 2.0 ** -149).astype(f32)             # subnormal f32
    assert np.all(np.abs(sub) < np.finfo(f32).tiny) and np.any(sub != 0)
    return np.concatenate([T, sub])


def test_area_and_weight_match_model_bitwise(host_exe, tmp_path):
    T = _triangles(np.random.default_rng(5))
    got = _run(host_exe, "area", T.reshape(-1, 9), tmp_path, f64).reshape(-1, 4)
    n, a2 = S.tri_normals_abc(*[T[:, k].astype(f64) for k in range(3)])
    want = np.concatenate([n, a2[:, None]], 1)
    assert np.array_equal(got.view(u64), want.view(u64))
    assert np.all(np.isfinite(got)) and np.count_nonzero(a2 == 0) >= 100 and np.count_nonzero(a2 > 0) >= 400
    # weights against the largest area of three groups of very different scale, and the quantisation's own edges
    rows = []
    for grp in (a2[:400], a2[400:640], a2[-40:]):
        rows += [(x, grp.max()) for x in grp]
    rows += [(1.0, 1.0), (2.0 ** -64, 1.0), (np.nextafter(2.0 ** -64, 0), 1.0), (2.0 ** -62, 1.0), (0.0, 1.0), (5e-324, 1.0), (0.25, 1.0),
             (np.nextafter(1.0, 0), 1.0), (3e-300, 7e-300)]
    rows = np.array(rows, f64)
    w = _run(host_exe, "weight", rows, tmp_path, u64)
    assert np.array_equal(w, S.weight(rows[:, 0], rows[:, 1]))
    k = len(rows) - 9
    assert list(w[k:k + 7]) == [1 << 32, 1, 0, 2, 0, 0, 1 << 31] and w.max() == 1 << 32


def test_draws_match_model_and_python_ints(host_exe, tmp_path):
    rng = np.random.default_rng(6)
    seeds = np.concatenate([np.array([0, 2 ** 64 - 1, 1, 2 ** 63], u64), rng.integers(0, 2 ** 64, 60, dtype=u64)])
    s = np.concatenate([np.array([0, 1, 2 ** 31 - 2, 2 ** 31 - 1], u64), rng.integers(0, 2 ** 31, 60, dtype=u64)])
    rows = np.stack([np.repeat(seeds, len(s)), np.tile(s, len(seeds))], 1)
    got = _run(host_exe, "draw", rows, tmp_path, u64).reshape(-1, 3)
    want = np.stack([np.concatenate([S.draws(sd, s)[j] for sd in seeds]) for j in range(3)], 1)
    assert np.array_equal(got, want)
    M = (1 << 64) - 1

    def mix(z):
        z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 & M
        z ^= z >> 27; z = z * 0x94D049BB133111EB & M
        return z ^ (z >> 31)
    for (sd, si), h in list(zip(rows.tolist(), got.tolist()))[::97]:
        assert h == [mix((sd + (3 * si + j + 1) * 0x9E3779B97F4A7C15) & M) for j in range(3)]


def test_pick_matches_model_and_exact_integers(host_exe, tmp_path):
    """Both modes at n = 1, 3, 100003 and 2^31 - 1 and totals from 5 (fewer units than samples: empty strata) to 2^63 - 1."""
    rng = np.random.default_rng(8)
    rows = []
    for n in (1, 3, 100003, 2 ** 31 - 1):
        for total in (5, 2 ** 32, 5000 * 2 ** 32 - 12345, 2 ** 63 - 1):
            s = np.unique(np.concatenate([[0, n - 1, n // 2], rng.integers(0, n, 20)]))
            for strat in (0, 1):
                h0 = rng.integers(0, 2 ** 64, len(s), dtype=u64)
                h0[0], h0[-1] = 0, 2 ** 64 - 1
                rows += [(int(h), int(si), n, total, strat) for h, si in zip(h0, s)]
    arr = np.array(rows, dtype=object).astype(u64)
    got = _run(host_exe, "pick", arr, tmp_path, u64)
    for (h, s, n, total, strat), r in zip(rows, got.tolist()):
        lo, hi = (s * total // n, (s + 1) * total // n) if strat else (0, total)
        assert r == lo + (h * (hi - lo) >> 64) and r < total, (h, s, n, total, strat, r)
        want = S.pick(np.array([h], u64), np.array([s], u64), n, total, bool(strat))[0]
        assert r == int(want)


def test_find_triangle_matches_searchsorted(host_exe, tmp_path):
    rng = np.random.default_rng(9)
    for nt in (1, 2, 5, 1000):
        w = rng.integers(0, 2 ** 32 + 1, nt, dtype=u64)
        w[rng.random(nt) < 0.3] = 0
        w[rng.integers(0, nt)] = 2 ** 32
        if nt >= 5:
            w[0] = w[-1] = 0
        W = np.zeros(nt + 1, u64)
        W[1:] = np.cumsum(w, dtype=u64)
        total = int(W[-1])
        r = np.unique(np.concatenate([W[:-1][w > 0], (W[1:] - u64(1))[w > 0], rng.integers(0, total, 200, dtype=u64)]))
        got = _run(host_exe, "find", np.concatenate([np.array([nt], u64), W, r]), tmp_path, np.int64)
        want = np.searchsorted(W[1:], r, side="right")
        assert np.array_equal(got, want)
        assert np.all(w[got] > 0) and np.all(W[got] <= r) and np.all(r < W[got + 1])
    # fewer units than samples (total < n): every stratified pick is still a valid position
    W = np.array([0, 0, 2, 2, 5], u64)
    s = np.arange(1000, dtype=u64)
    r = S.pick(S.draws(3, s)[0], s, 1000, 5, True)
    assert np.all(r < 5)
    got = _run(host_exe, "find", np.concatenate([np.array([4], u64), W, r]), tmp_path, np.int64)
    assert set(got.tolist()) == {1, 3} and np.array_equal(got, np.searchsorted(W[1:], r, side="right"))


SAMPLE_IN = np.dtype([("tri", f32, 9), ("pad", f32), ("h", u64, 2)])
SAMPLE_OUT = np.dtype([("o", f32, 9), ("pad", f32), ("w", f64, 3)])
FOLD_EDGES = [(ONE53 // 2, ONE53 // 2), (ONE53 // 2 + 1, ONE53 // 2), (0, 0), (ONE53 - 1, ONE53 - 1), (ONE53 - 1, 1), (ONE53 - 1, 2), (0, ONE53 - 1)]


def test_samples_match_model_bitwise(host_exe, tmp_path):
    rng = np.random.default_rng(10)
    T = _triangles(rng)
    _, a2 = S.tri_normals_abc(*[T[:, k].astype(f64) for k in range(3)])
    T = T[a2 > 0]                                    # (only a triangle with an area is ever sampled)
    assert len(T) >= 500
    h = rng.integers(0, 2 ** 64, (len(T), 2), dtype=u64)
    edges = np.array(FOLD_EDGES, dtype=object).astype(u64) << u64(11)
    edges[::2] |= u64(0x7FF)                           # (the low 11 bits are dropped)
    rows = np.zeros(len(T) + len(edges) * 3, SAMPLE_IN)
    rows["tri"] = np.concatenate([T, np.repeat(T[[0, 420, len(T) - 1]], len(edges), 0)]).reshape(-1, 9)
    rows["h"] = np.concatenate([h, np.tile(edges, (3, 1))])
    got = _run(host_exe, "sample", rows, tmp_path, SAMPLE_OUT)
    tri = rows["tri"].reshape(-1, 3, 3)
    P, Nn, wf, w, k = S.sample_on(tri[:, 0], tri[:, 1], tri[:, 2], rows["h"][:, 0], rows["h"][:, 1])
    want = np.concatenate([P, Nn, wf], 1)
    assert np.array_equal(got["o"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got["w"].view(u64), w.view(u64))
    assert np.all(np.isfinite(got["o"]))
    # the fold's edge cases, as integers
    ke = k[len(T):len(T) + len(edges)].tolist()
    assert ke[0] == [0, ONE53 // 2, ONE53 // 2] and ke[1] == [1, ONE53 // 2 - 1, ONE53 // 2] and ke[2] == [ONE53, 0, 0]
    assert ke[3] == [ONE53 - 2, 1, 1] and ke[4] == [0, ONE53 - 1, 1] and ke[5] == [1, 1, ONE53 - 2]
    assert np.all(k.sum(1) == ONE53) and np.all(k <= ONE53)
    assert np.array_equal(w, k.astype(f64) / f64(ONE53)) and np.all((w[:, 0] + w[:, 1]) + w[:, 2] == 1.0)


# ---- invariants of the model on recorded meshes ---------------------------------------------------------------------------
def _mesh(name):
    base, _, off = name.partition("+")
    V, T = SMALL[base + ".vertices"], SMALL[base + ".triangles"]
    return (V + f32(float(off))) if off else V, T


@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("name", ["Sphere10", "ColoredSpheres", "Sphere5+65536"])
def test_model_invariants_on_recorded_meshes(name, stratified):
    V, T = _mesh(name)
    n = 20011
    w, W = S.weights(V, T)
    total = int(W[-1])
    R = S.sample(V, T, n, seed=12, stratified=stratified)
    assert np.all(R.k[:, 0] <= u64(ONE53)) and np.all(R.k.sum(1) == u64(ONE53))          # k0 >= 0 (unsigned: no wrap)
    assert np.all(w[R.Triangles] > 0) and R.Triangles.min() >= 0 and R.Triangles.max() < len(T) // 3
    count = np.bincount(R.Triangles, minlength=len(w))
    if stratified:
        worst = max(abs(int(c) * total - n * int(wt)) for c, wt in zip(count, w))
        assert worst < 2 * total, worst / total
        assert np.all(np.diff(R.Triangles) >= 0)                                         # the output follows the triangle order
    Vd = V.astype(f64)
    Tt = T.reshape(-1, 3)[R.Triangles]
    a, b, c = Vd[Tt[:, 0]], Vd[Tt[:, 1]], Vd[Tt[:, 2]]
    d2, _, _ = MM.closest_on_triangle(R.Points.astype(f64), a, b, c)
    M = np.max(np.abs(np.concatenate([a, b, c], 1)), 1)
    ratio = np.sqrt(d2) / (2.0 ** -23 * M)
    print(name, stratified, "worst distance / (2^-23 M)", ratio.max())
    assert ratio.max() <= 1.0
    lens = np.sqrt(np.sum(R.Normals.astype(f64) ** 2, 1))
    assert np.all(np.abs(lens - 1) < 1e-6)


@pytest.mark.parametrize("name", [k[:-9] for k in SMALL.files if k.endswith(".vertices") and len(SMALL[k])])
def test_face_normals_agree_in_sign_with_the_marching_cubes_vertex_normals(name):
    """On every triangle of every recorded mesh, the face normal of the winding (b - a) x (c - a) points to the side of each of its
    vertices' normals (where the triangle has an area and the vertex normal is not zero)."""
    V, T, Nv = SMALL[name + ".vertices"], SMALL[name + ".triangles"].reshape(-1, 3), SMALL[name + ".normals"].astype(f64)
    n, a2 = S.tri_normals(V, T)
    ok = a2 > 0
    for k in range(3):
        dots = np.sum(n[ok] * Nv[T[ok, k]], 1)
        assert np.all(dots[np.any(Nv[T[ok, k]] != 0, 1)] > 0), (name, k, np.count_nonzero(dots <= 0))


def test_zero_weight_triangles_are_never_returned():
    """The weight-quantisation mesh and the one with zero-area triangles first, last and in between."""
    V, T = Cs.weight_quantisation()
    w, W = S.weights(V, T)
    assert sorted(set(w.tolist())) == [0, 1, 1 << 32]
    for strat in (False, True):
        R = S.sample(V, T, 50000, seed=1, stratified=strat)
        assert np.all(w[R.Triangles] > 0)
    V, T = Cs.degenerate_interleaved()
    w, W = S.weights(V, T)
    assert np.all(w[::2] == 0) and w[39] == 0 and np.all(w[1:39:2] > 0)
    R = S.sample(V, T, 50000, seed=1, stratified=True)
    assert np.all(w[R.Triangles] > 0) and set(R.Triangles.tolist()) == set(range(1, 39, 2))
    assert S.weights(*Cs.all_degenerate()) == (None, None)

