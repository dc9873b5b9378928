"""The meshes of the mesh stress tests (tests/test_mesh_stress_cases.py on the CPU, tests/test_gpu_mesh_stress.py on the device):
inputs that the tidy, hand-made meshes of tests/mesh_topology_cases.py, mesh_smooth_cases.py, mesh_weld_cases.py and
mesh_sample_cases.py never give the mesh units -- random index soups, runs of one edge, one vertex's neighbours, one vertex's
corners and one weld group that are longer than a 2048-record sort tile, more than 65 536 components, and sums whose float32
result is decided by the order of the adds.  Not a test module.

Every mesh is (V (nv, 3) float32, T (nt, 3) int32).  Every random number is an integer drawn from a seeded np.random.default_rng
(or a permutation), and every coordinate is such an integer times a power of two (the books' rings: a quotient of small
integers in binary64, rounded once), so the positions are the same bits on every machine.  The numpy models
(tests/mesh_topology_model.py, mesh_smooth_model.py, mesh_weld_model.py, mesh_sample_model.py) are the yardstick of every one."""
import functools

import numpy as np

from tests.mesh_topology_cases import permuted

f32, f64, i32, i64 = np.float32, np.float64, np.int32, np.int64

SOUP_SEEDS = tuple(range(64))
ARCHIPELAGO_SEEDS = tuple(range(1000, 1300))     # (other seeds than the soups')
_STREAM = 0x6D657368                             # the first word of every seed sequence here


def _frozen(V, T):
    V, T = np.ascontiguousarray(V, f32), np.ascontiguousarray(T, i32)
    V.setflags(write=False)
    T.setflags(write=False)
    return V, T


# ---- 1. index soups -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup(seed):
    """nv in [3, 40) vertices on the lattice 0.25 * [-4, 4]^3, each zero coordinate -0.0 with probability 1/2, and nt in [1, 120)
    uniformly random index triples (so index-degenerate triangles, repeated edges of every multiplicity and equal positions all
    occur); one soup in four has few triangles for its vertices, so several components and unreferenced vertices.  One soup in
    four also lists some of its triangles again: as they are, rotated, and reversed."""
    rng = np.random.default_rng([_STREAM, 1, seed])
    nv, nt = int(rng.integers(3, 40)), int(rng.integers(1, 120))
    if int(rng.integers(0, 4)) == 0:
        nt = 1 + nt % max(nv // 3, 1)
    k = rng.integers(-4, 5, (nv, 3))
    V = (k.astype(f64) * 0.25).astype(f32)
    V[(k == 0) & (rng.integers(0, 2, (nv, 3)) == 1)] = f32(-0.0)
    T = rng.integers(0, nv, (nt, 3))
    if int(rng.integers(0, 4)) == 0:
        again = T[rng.integers(0, nt, int(rng.integers(1, 9)))]
        T = np.concatenate([T, again, again[:, [1, 2, 0]], again[:, ::-1]])
    return _frozen(V, T)


@functools.lru_cache(maxsize=None)
def archipelago():
    """300 soups laid over each other: concatenated with index offsets only, so the components share positions; then the vertex
    indices are permuted and the triangles shuffled."""
    Vs, Ts, base = [], [], 0
    for seed in ARCHIPELAGO_SEEDS:
        V, T = soup(seed)
        Vs.append(V)
        Ts.append(T.astype(i64) + base)
        base += len(V)
    return _frozen(*permuted(np.concatenate(Vs), np.concatenate(Ts), 17))


# ---- 2. one long run: the books -------------------------------------------------------------------------------------------------
def _quarter_circle(n):
    """n + 1 points of the unit quarter circle by its rational parametrisation (no libm), as mesh_smooth_cases.big_fan."""
    t = np.arange(n + 1).astype(f64) / f64(n)
    return (1 - t * t) / (1 + t * t), 2 * t / (1 + t * t)


@functools.lru_cache(maxsize=None)
def book(n, reversed_every):
    """n pages (0, 1, 2 + k) on the one spine edge (0, 1); every reversed_every-th page (k % reversed_every == 0) is listed as
    (1, 0, 2 + k), none when reversed_every is 0.  The spine runs from (0, 0, 0) to (0, 0, 1); the ring lies on a quarter circle.
    The spine is one run of n edge records out of 3 n; each hub has n + 1 neighbours from 2 n of the 6 n neighbour records, and n of
    the 3 n corner records."""
    x, y = _quarter_circle(n)
    k = np.arange(n)
    ring = np.stack([x[:n], y[:n], f64(0.001) * (k % 7) + 0.25], 1)
    V = np.concatenate([np.array([[0, 0, 0], [0, 0, 1]], f64), ring]).astype(f32)
    T = np.stack([np.zeros(n, i64), np.ones(n, i64), 2 + k], 1)
    if reversed_every:
        rev = k % reversed_every == 0
        T[rev] = T[rev][:, [1, 0, 2]]
    return _frozen(V, T)


BOOKS = {"odd_4999": (4999, 3), "even_5000": (5000, 3), "two_pages": (2, 0)}
# census (components, vertices, edges, boundary, non-manifold, odd, inconsistent, degenerate)
BOOK_CENSUS = {"odd_4999": [1, 5001, 9999, 9998, 1, 9999, 0, 0], "even_5000": [1, 5002, 10001, 10000, 1, 10000, 0, 0],
               "two_pages": [1, 4, 5, 4, 0, 4, 1, 0]}

CANCELLING_HALF = 1500
# The ring radii: 24-bit integers times 2^(e - 24), e from here.  The narrowest symmetric spread at which the model's position sums
# round, so that descending order changes the hubs' smoothed bits: at (-12, 0, 12) every partial sum of 3000 such terms still fits
# the binary64 significand and the residue is exactly 0 (tried with three seeds each; the crosses' sums round already at (-8, 0, 8)).
CANCELLING_SCALES = (-13, 0, 13)


@functools.lru_cache(maxsize=None)
def cancelling_book(h=CANCELLING_HALF, scales=CANCELLING_SCALES, seed=5):
    """A book of 2 h pages whose hubs' sums cancel.  The hubs lie on the z axis at heights that are no short binary fractions;
    ring vertex j of the first half lies at (x, y, z) with x and y 24-bit integers times 2^(e - 24), e drawn from `scales`, and
    its partner of the second half at (-x, -y, z).  The face cross of a page (0, 1, v) is (-dz y, dz x, 0), dz the spine's length,
    so the exact sum of the crosses at either hub is (0, 0, 0), and so is the exact sum of the ring's positions in x and y: what a
    hub's binary64 sums leave in x and y is the rounding of their partial sums, which depends on the order of the adds, and that
    residue alone decides the hub's float32 normal and the x and y of its smoothed position.  (With the radii in one binade and
    the hubs at 0 and 1 every partial sum is exact, the residue 0, and the case shows nothing: the products must fill the
    binary64 significand and the radii span enough binades.)  The ring's indices are permuted, so that ascending neighbour order
    is not the order of generation, and no page is reversed."""
    rng = np.random.default_rng([_STREAM, 2, seed])
    e = np.asarray(scales)[rng.integers(0, len(scales), h)]
    xy = rng.integers(-(1 << 24) + 1, 1 << 24, (h, 2)).astype(f64) * (2.0 ** (e - 24.0))[:, None]
    z = rng.integers(-(1 << 20), 1 << 20, h).astype(f64) * 2.0 ** -20
    half = np.concatenate([xy, z[:, None]], 1)
    ring = np.concatenate([half, half * np.array([-1.0, -1.0, 1.0])])
    ring = ring[rng.permutation(2 * h)]
    V = np.concatenate([np.array([[0, 0, 0.3], [0, 0, 1.7]], f32).astype(f64), ring]).astype(f32)
    assert np.array_equal(V[2:].astype(f64), ring)                      # every ring coordinate is exact in float32
    T = np.stack([np.zeros(2 * h, i64), np.ones(2 * h, i64), 2 + np.arange(2 * h)], 1)
    return _frozen(V, T)


# ---- 3. more components than 65 536 ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loose_triangles(count=70000, seed=6):
    """`count` triangles without a shared vertex over a random permutation of the 3 * count indices: `count` components.
    Triangle k sits in cell k of a coarse lattice (64 cells a row, 64 rows a layer, spacing 1), a small right triangle whose legs
    grow with k % 5, so each triangle is small against the whole and the handle's closest-point grid stays small."""
    rng = np.random.default_rng([_STREAM, 3, seed])
    k = np.arange(count)
    base = np.stack([k % 64, (k // 64) % 64, k // 4096], 1).astype(f64)
    leg = 0.125 * (1 + k % 5).astype(f64)
    corners = np.stack([base, base + np.stack([leg, 0 * leg, 0 * leg], 1), base + np.stack([0 * leg, leg, 0.25 + 0 * leg], 1)], 1)   # (count, 3, 3)
    perm = rng.permutation(3 * count)
    V = np.empty((3 * count, 3), f64)
    V[perm] = corners.reshape(-1, 3)
    T = perm.reshape(count, 3)[rng.permutation(count)]
    return _frozen(V, T)


# ---- 4. one weld group longer than two sort tiles -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_big_group(nv=6200, others=150, nt=4000, seed=7):
    """nv vertices, all but `others` at (+-0, 0.5, -0.75) -- one position as values, -0.0 and +0.0 mixed in x -- and `others` on
    the integer lattice [0, 4)^3, scattered through the index range; nt uniformly random triangles."""
    rng = np.random.default_rng([_STREAM, 4, seed])
    V = np.empty((nv, 3), f32)
    V[:] = [0.0, 0.5, -0.75]
    V[rng.integers(0, 2, nv) == 1, 0] = f32(-0.0)
    at = rng.permutation(nv)[:others]
    V[at] = rng.integers(0, 4, (others, 3)).astype(f32)
    return _frozen(V, rng.integers(0, nv, (nt, 3)))


# ---- 5. the cell faces at zero and below ----------------------------------------------------------------------------------------
NEGATIVE_FACES_TOLERANCE = 0.25
FACE_KS = tuple(range(-3, 4))


@functools.lru_cache(maxsize=None)
def negative_faces(tolerance=NEGATIVE_FACES_TOLERANCE):
    """On each axis, for k in -3 .. 3: the vertex whose coordinate on that axis is k * tolerance (the face between the cells k - 1
    and k of the lattice), the one a float32 below it and the one a float32 above it (around zero: the least subnormals), and
    after them the vertex with -0.0 there; the other two coordinates are half a cell, tolerance / 2.  Vertex 22 a + 3 (k + 3) + s
    is axis a, face k, s = 0 on the face, 1 below it, 2 above it; vertex 22 a + 21 holds the -0.0.  22 triangles over consecutive
    indices name every vertex."""
    t = f32(tolerance)
    V = []
    for a in range(3):
        values = []
        for k in FACE_KS:
            c = f32(k) * t
            values += [c, np.nextafter(c, f32(-np.inf)), np.nextafter(c, f32(np.inf))]
        for c in values + [f32(-0.0)]:
            p = [t * f32(0.5)] * 3
            p[a] = c
            V.append(p)
    V = np.array(V, f32)
    return _frozen(V, np.arange(len(V)).reshape(-1, 3))


def face_vertex(axis, k, s):
    """The index in negative_faces() of the vertex of `axis` at face k: s = 0 on it, 1 the float32 below, 2 the float32 above."""
    return 22 * axis + 3 * (k - FACE_KS[0]) + s


def minus_zero_vertex(axis):
    return 22 * axis + 21
