"""The meshes of the simplification stress tests (tests/test_mesh_simplify_stress_cases.py on the CPU,
tests/test_gpu_mesh_simplify_stress.py on the device): inputs the hand-made meshes of tests/mesh_simplify_cases.py never give
sdfk_trimesh_simplify -- centroids whose float32 bits are decided by the order and the chunking of the adds, quadrics whose
minimiser lies on a cell face in exact arithmetic so that rounding decides its side, one kept group of more than two sort tiles and one vertex of 3000 corners
inside 65 535 / 65 537 groups, runs of 4999 / 5000 / 5001 equal vertex sets, group counts on both sides of every byte of the
group number, triangle counts independent of the vertex count, fallbacks placed lane by lane, minimisers that land exactly on a
cell face, an eigenvalue exactly at the truncation, and coordinates at both ends of the float32 range.  Not a test module.

A case is (V (nv, 3) float32, T (nt, 3) int32, colors (nv, 3) float32 or None, cellSize), frozen.  Every coordinate is an exact
binary fraction (asserted: the float64 it is written as survives the rounding to float32) or an integer of a seeded generator
times a power of two, so the bits are the same on every machine.  What each case is there for is proved from the numpy model
(tests/mesh_simplify_model.py) alone in tests/test_mesh_simplify_stress_cases.py."""
import functools

import numpy as np

from tests.mesh_simplify_cases import CHUNK, TILE, corner
from tests.mesh_topology_cases import patch

f32, f64, i32, i64 = np.float32, np.float64, np.int32, np.int64
_STREAM = 0x73696D70                             # the first word of every seed sequence here


def _frozen(V, T, cols, cell):
    V, T = np.ascontiguousarray(V, f32), np.ascontiguousarray(np.asarray(T).reshape(-1, 3), i32)
    V.setflags(write=False)
    T.setflags(write=False)
    if cols is not None:
        cols = np.ascontiguousarray(cols, f32)
        cols.setflags(write=False)
    return V, T, cols, cell


def _exact(P):
    """float64 coordinates that are float32 values already."""
    P = np.asarray(P, f64).reshape(-1, 3)
    assert np.array_equal(P.astype(f32).astype(f64), P)
    return P.astype(f32)


class _Mesh:
    """Vertices and triangles collected piece by piece."""

    def __init__(self):
        self.P, self.T, self.n = [], [], 0

    def v(self, pts):
        pts = np.asarray(pts, f64).reshape(-1, 3)
        first = self.n
        self.P.append(pts)
        self.n += len(pts)
        return np.arange(first, self.n)

    def t(self, tris):
        self.T.append(np.asarray(tris, i64).reshape(-1, 3))

    def arrays(self):
        return _exact(np.concatenate(self.P)), (np.concatenate(self.T) if self.T else np.zeros((0, 3), i64))


def filler(count, z=-8.0):
    """`count` vertices no triangle names, one per cell of the lattice 1, 256 a row, in the layer z: `count` groups that are never
    kept (they give the number of groups its value and k_ts_place its idle lanes)."""
    k = np.arange(count)
    return np.stack([k % 256 + 0.5, k // 256 + 0.5, np.full(count, z + 0.5)], 1)


# ---- A. centroids decided by the order of the adds -----------------------------------------------------------------------------
TINY = 2.0 ** -51
CENTROID_SIZES = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)


def midpoint_column(n, at, k, odd=1, tiny=TINY):
    """n values of [0, 1), in index order, whose exact sum is n (1/2 + odd 2^-25) + k TINY: the exact mean lies k TINY / n above
    the midpoint of two neighbouring float32 values (ON it for k = 0).  k of the values are TINY, at the indices at .. at + k - 1;
    the others are n - k - 1 multiples of 1/64 near 2/3 and the one value 1/4 + odd n 2^-25.  Every partial sum of the others is
    exact in binary64 (multiples of 2^-25 below 64); a TINY added to a sum of 8 or more is lost (it is below half an ulp), k of
    them added to each other first are not: k TINY is an ulp or more of the total.  So the order of the adds decides on which
    side of the midpoint the binary64 mean falls, and the float32 result with it."""
    m = n - k - 1
    units = int((n / 2 - 0.25) * 64)
    q, r = divmod(units, m)
    assert 32 <= q and q + 1 < 64
    big = [(q + 1) / 64.0] * r + [q / 64.0] * (m - r) + [0.25 + odd * n * 2.0 ** -25]
    big = big[1::2] + big[0::2]                                   # (ascending index is not ascending magnitude)
    out = big[:at] + [tiny] * k + big[at:]
    assert len(out) == n and all(0 <= x < 1 for x in out)
    return np.array(out, f64)


@functools.lru_cache(maxsize=None)
def centroid_order(n):
    """One group of n members in the cell [0, 1)^3, kept (every member is a corner of a triangle to the two anchors' groups), with
    colours.  x: the TINY members come FIRST (ascending: they survive, the mean rounds up; descending: lost, the tie rounds to
    even).  y: they open the SECOND chunk when there is one (chunks of 32: they survive; one running sum or chunks of 64: lost),
    else they come last.  z: no TINY member, the exact mean ON the midpoint 1/2 + 3 2^-25 (a tie, rounded to even); for 31
    members one member of 2^-49 instead, an ulp of the sum 15.5, so that the sum is exact in EVERY order and lies 0.516 ulp of the
    mean above 31 midpoints: the division rounds up, the product with the rounded 1 / 31 (0.125 ulp less) rounds down onto the
    tie.  Colours: the same columns in another order, one negated, one scaled by 4."""
    k = 8 if n <= CHUNK + 1 else 16
    x = midpoint_column(n, 0, k)
    y = midpoint_column(n, CHUNK if n >= 2 * CHUNK + 1 else n - k, k)
    z = midpoint_column(n, 1, 1, tiny=2.0 ** -49) if n == CHUNK - 1 else midpoint_column(n, 0, 0, odd=3)
    M = _Mesh()
    g = M.v(np.stack([x, y, z], 1))
    a = M.v([(2.5, 0.5, 0.5), (0.5, 2.5, 0.5)])
    M.t(np.stack([g, np.full(n, a[0]), np.full(n, a[1])], 1))
    V, T = M.arrays()
    cols = np.concatenate([np.stack([y, -x, 4.0 * z], 1), [(0.5, 0.25, 0.125), (0.25, 0.5, 1.0)]])
    return _frozen(V, T, _exact(cols), 1.0)


# ---- B. quadrics decided by the order of the adds --------------------------------------------------------------------------------
KNIFE_SEEDS = (496, 110, 171, 102, 0, 3)
KNIFE_MOVED_BY = {"corners_descending": (0, 2), "straight_into_chunk": (1, 3, 5)}
KNIFE_GROUPS = len(KNIFE_SEEDS)
KNIFE_MEMBERS = CHUNK + 8
KNIFE_CORNERS = 6


def knife_group(M, i, seed):
    """Group i of knife_edge from its own seed -> its triangles."""
    rng = np.random.default_rng([_STREAM, 2, seed])
    P = np.array([4 * i + 1, 0.5, 0.5])
    m = np.array([4 * i, 0, 0]) + rng.integers(1, 16, (KNIFE_MEMBERS, 3)).astype(f64) / 16
    g, tris = M.v(m), []
    for j, v in enumerate(g):
        for r in range(KNIFE_CORNERS):
            w = np.r_[rng.integers(-4, 5, 2), rng.integers(1, 5)].astype(f64) * (1 << int(rng.integers(0, 6)))
            a, b = M.v([3 * P - 2 * m[j], P + w])
            tris.append([(v, a, b), (a, b, v), (b, v, a)][(j + r) % 3])
    return tris


@functools.lru_cache(maxsize=None)
def knife_edge(seeds=None):
    """6 groups of 40 members, group i in the cell (4 i, 0, 0) of the lattice 1, members on sixteenths.  EVERY plane of a group
    passes through the one point P = (4 i + 1, 1/2, 1/2) ON the upper x face of its cell: a member m has six triangles
    (m, 3 P - 2 m, P + s w), w of small integers with w_z >= 1, s a power of two up to 32 -- all exact in float32 and exactly
    coplanar with P (asserted in integers on the CPU).  The quadric has rank 3 and in exact arithmetic its minimiser IS P:
    p_x = the upper face, outside, a fallback.  In binary64 (the mean of 40 members is rounded, and every q with it) p_x is the
    face plus or minus some ulps, and its SIGN -- the placement or the centroid, and the fallback count -- is decided by
    rounding.  Most of that is the rounding inside a triangle's own terms, which no order changes; so the seeds are CHOSEN
    (KNIFE_SEEDS, found by trying seeds on the numpy model in order, per cell) for groups that land so close to the face that
    the order of a member's corners (groups 0 and 2) or adding the terms straight into the chunk without the member's own sum
    (groups 1, 3 and 5) moves them across it (KNIFE_MOVED_BY).  A contracted multiply-subtract in the normal and a q taken from the rounded centroid move several."""
    M = _Mesh()
    tris = []
    for i, seed in enumerate(KNIFE_SEEDS if seeds is None else seeds):
        tris += knife_group(M, i, seed)
    M.t(tris)
    V, T = M.arrays()
    return _frozen(V, T, None, 1.0)


@functools.lru_cache(maxsize=None)
def shared_corners():
    """One group of three members in the cell [0, 1)^3 whose planes do NOT meet in a point, so that the weights of the triangles
    move the minimiser: one triangle has all three members as corners (it counts three times), one has two (twice), three have
    one.  Counting a triangle once per group instead gives another vertex."""
    M = _Mesh()
    g = M.v([(0.25, 0.5, 0.5), (0.5, 0.25, 0.5), (0.5, 0.5, 0.25)])
    f = M.v([(0.5, 0.625, 3.5), (2.5, 0.5, 0.375), (0.5, 2.5, 0.5), (3.5, 3.5, 0.25), (-1.5, 0.5, 0.75)])
    M.t([(g[0], g[1], g[2]), (g[0], g[1], f[0]), (g[2], f[1], f[2]), (g[1], f[3], f[1]), (g[0], f[2], f[4]), (f[0], f[1], f[3])])
    V, T = M.arrays()
    return _frozen(V, T, None, 1.0)


# ---- C. large kept groups inside 64 k +- 1 groups ---------------------------------------------------------------------------------
BIG_MEMBERS = 2 * TILE + 100
HUB_CORNERS = 3000
HUB_MATES = 3


@functools.lru_cache(maxsize=None)
def large_groups(groups, seed=3):
    """`groups` groups in all.  One KEPT group of 2 TILE + 100 members in the cell (0, 0, 0) (20-bit fractions of a seeded
    generator; every member a corner of a triangle to the same two other groups); one hub in the cell (4, 0, 0): a vertex with
    3000 incident corners, a fan whose 3000 rim vertices lie in 3000 other cells, and three cell-mates of one triangle each; the
    rest filler.  The vertex indices are permuted and the triangles shuffled, with colours."""
    rng = np.random.default_rng([_STREAM, 3, seed])
    M = _Mesh()
    big = M.v(rng.integers(1, 1 << 20, (BIG_MEMBERS, 3)).astype(f64) * 2.0 ** -20)
    a = M.v([(2.5, 0.5, 0.5), (0.5, 2.5, 0.5)])
    M.t(np.stack([big, np.full(BIG_MEMBERS, a[0]), np.full(BIG_MEMBERS, a[1])], 1))
    hub = M.v([(4.5, 0.5, 0.25)])[0]
    mates = M.v(np.array([4, 0, 0], f64) + rng.integers(1, 1 << 20, (HUB_MATES, 3)).astype(f64) * 2.0 ** -20)
    j = np.arange(HUB_CORNERS)
    rim = M.v(np.stack([8 + j % 60 + 0.5, 2 + j // 60 + 0.5, 1.0 + (rng.integers(0, 1 << 10, HUB_CORNERS)).astype(f64) * 2.0 ** -10], 1))
    M.t(np.stack([np.full(HUB_CORNERS, hub), rim, np.roll(rim, -1)], 1))
    M.t(np.stack([mates, rim[:HUB_MATES], rim[7:7 + HUB_MATES]], 1))
    made = 1 + 2 + 1 + HUB_CORNERS
    M.v(filler(groups - made))
    V, T = M.arrays()
    perm = rng.permutation(len(V))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(V))
    V, T = V[perm], inv[T][rng.permutation(len(T))]
    cols = (rng.integers(-(1 << 12), 1 << 12, (len(V), 3)).astype(f64) * 2.0 ** rng.integers(-20, 8, (len(V), 1))).astype(f32)
    return _frozen(V, T, cols, 1.0) + ((int(inv[hub]), inv[big], inv[mates]),)


# ---- D. long runs of equal vertex sets ----------------------------------------------------------------------------------------------
RUNS = (4999, 5000, 5001)
RUN_SETS = ((3, 7, 11), (4, 9, 2), (12, 5, 8))         # (a, b, c) of the three runs: vertex = group number
DEGENERATE_RUN = 3001
ZERO_LO_RUN = 2000                                       # copies of the set (0, 6, 10): its lo is group 0, next to the degenerate records
FAMILY = {"lo": [(13, 20, 21), (14, 20, 21), (15, 20, 21)], "mid": [(13, 17, 22), (13, 18, 22), (13, 19, 22)],
          "hi": [(14, 16, 23), (14, 16, 24), (14, 16, 25)]}
_WINDINGS = ((1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2))   # of the copies between the first (0, 1, 2) and the last (2, 1, 0)


def run_triangle(s, j, n):
    """Copy j of n of the set s = (a, b, c): the first is (a, b, c), the last (c, b, a), and no copy between them has either
    winding -- so the corners of the kept triangle say which copy it was."""
    w = (0, 1, 2) if j == 0 else (2, 1, 0) if j == n - 1 else _WINDINGS[j % 4]
    return tuple(s[k] for k in w)


@functools.lru_cache(maxsize=None)
def long_runs():
    """27 vertices: 26 in cells of their own (vertex = group number) and vertex 26 in the cell of vertex 25.  The triangles:
    920 strips first; then the three runs of 4999, 5000 and 5001 copies, 3001 degenerate triangles (index-degenerate ones, and
    every fourth (25, 26, k): two corners in one group) and 2000 copies of a set whose lo is group 0 -- next to the degenerate
    records after the sorts -- dealt round-robin; then the three families (sets that differ only in lo, only in mid, only in
    hi; each set twice, the copies nine apart); then 230 strips wound the other way.  The lowest index of every run lies
    inside the array, after the 920.  -> the case and {stream: (first index, last index, count)}."""
    M = _Mesh()
    k = np.arange(26)
    M.v(np.stack([2.0 * (k % 8) + 0.5, 2.0 * (k // 8) + 0.5, 0.25 + 0 * k], 1))
    M.v([(2.0 * (25 % 8) + 0.75, 2.0 * (25 // 8) + 0.25, 0.5)])
    head = [(k, k + 1, k + 2) for k in range(0, 23)] * 40                     # 920 triangles before the runs: sets met again and again
    streams = {i: [run_triangle(RUN_SETS[i], j, n) for j in range(n)] for i, n in enumerate(RUNS)}
    streams["deg"] = [((j % 25) + 1, (j % 25) + 1, j % 7) if j % 2 else (25, 26, j % 25) if j % 4 == 0 else (j % 26, (j + 3) % 26, j % 26)
                      for j in range(DEGENERATE_RUN)]
    streams["zero"] = [run_triangle((0, 6, 10), j, ZERO_LO_RUN) for j in range(ZERO_LO_RUN)]
    T, where = list(head), {}
    left = {n: 0 for n in streams}
    while any(left[n] < len(s) for n, s in streams.items()):
        for n, s in streams.items():
            if left[n] < len(s):
                where.setdefault(n, [len(T), len(T), 0])
                where[n][1] = len(T)
                where[n][2] += 1
                T.append(s[left[n]])
                left[n] += 1
    fam = [s for name in ("lo", "mid", "hi") for s in FAMILY[name]]
    T += fam + [(s[1], s[2], s[0]) for s in fam]
    T += [(k + 2, k + 1, k) for k in range(0, 23)] * 10
    M.t(T)
    V, T = M.arrays()
    return _frozen(V, T, None, 1.0) + ({n: tuple(w) for n, w in where.items()},)


# ---- E. the bytes of the group number -----------------------------------------------------------------------------------------------
BYTE_EDGES = (2, 3, 255, 256, 257, 65535, 65536, 65537)


@functools.lru_cache(maxsize=None)
def byte_edge(groups):
    """`groups` vertices, one per cell, so that vertex = group number; the triangles name the group numbers directly.  With
    top = groups - 1 and B the value of the top byte's least bit (1, 256 or 65 536 as top has one, two or three bytes): pairs
    of sets that differ ONLY in the top byte of hi, of mid or of lo, each set three times, the copies dealt far apart (a block of
    strips between the rounds): a sort that ran one pass too few leaves the copies of the two sets interleaved, and no run forms.
    Where the top byte holds one group only (257, 65 537: top = B) no such pair exists -- its partner would be group 0 in
    another role -- and the sets name group `top` as hi only.  2 groups: three vertices in two cells, only degenerate triangles."""
    if groups == 2:
        return _frozen(_exact([(0.5, 0.5, 0.5), (0.25, 0.75, 0.5), (2.5, 0.5, 0.5)]), [(0, 1, 2), (2, 0, 1), (1, 1, 2), (0, 2, 2)], None, 1.0)
    top = groups - 1
    B = 1 if top < 256 else 256 if top < 65536 else 65536
    sets = []
    if groups == 3:
        sets = [(0, 1, 2)]
    elif top == B:
        sets = [(1, 2, top), (0, 2, top), (3, 4, top)]
    else:
        h = top // B * B                                              # the top byte at its highest value, the low bytes zero
        low = [5, 6, 7] if B > 1 else [0, 0, 0]
        if B == 1:                                                    # one byte: "the top byte" is the whole number
            sets = [(1, 2, top), (1, 2, top - 1), (1, top - 2, top), (1, top - 3, top), (top - 2, top - 1, top), (top - 3, top - 1, top)]
        else:
            sets = [(low[0], low[1], h + low[2]), (low[0], low[1], h - B + low[2]),                  # hi
                    (low[0], h + low[1], top), (low[0], h - B + low[1], top),                        # mid
                    (h + low[0], top - 1, top), (h - B + low[0], top - 1, top)]                      # lo
    strips = [(k, k + 1, k + 2) for k in range(0, min(groups - 2, 300))]
    T = []
    for round_ in range(3):
        T += [(s[round_ % 3], s[(round_ + 1) % 3], s[(round_ + 2) % 3]) if round_ != 1 else (s[1], s[0], s[2]) for s in sets]
        T += strips + [(0, 0, 1), (top, top, top)]
    k = np.arange(groups)
    V = np.stack([k % 256 + 0.5, (k // 256) % 256 + 0.5, k // 65536 + 0.5], 1)
    return _frozen(_exact(V), T, None, 1.0)


# ---- F. triangle counts independent of the vertex count ---------------------------------------------------------------------------
TRIANGLE_COUNTS = (255, 256, 257, 2047, 2048, 2049)


@functools.lru_cache(maxsize=None)
def many_triangles(nt, nv=12, seed=6):
    """nt uniformly random index triples over 12 vertices in 9 cells: duplicates of every multiplicity, degenerate ones."""
    rng = np.random.default_rng([_STREAM, 6, seed])
    V = rng.integers(0, 3 << 4, (nv, 3)).astype(f64) / 16.0
    V[:, 2] = V[:, 2] / 4.0
    return _frozen(_exact(V), rng.integers(0, nv, (nt, 3)), _exact(rng.integers(-64, 64, (nv, 3)) / 8.0), 1.0)


# ---- G. the fallback census -----------------------------------------------------------------------------------------------------
def _sheets(nx, ny, origin):
    """tests/mesh_simplify_cases.two_sheets over nx x ny cells of the lattice 1 (4 x 4 vertices of either sheet in every cell)."""
    V, T = patch(4 * nx - 1, 4 * ny - 1)
    A = np.stack([V[:, 0] * f32(0.5) + f32(0.125), V[:, 1] + f32(0.0625), np.full(len(V), 0.2, f32)], 1).astype(f32)
    B = A.copy()
    B[:, 2] = f32(0.3) + f32(0.2) * A[:, 0]
    both = np.concatenate([A, B]).astype(f64) + np.asarray(origin, f64)
    return both.astype(f32).astype(f64), np.concatenate([T, T + len(V)])


SHEET_TILES = {63: (21, 0), 64: (20, 2), 65: (19, 4), 257: (83, 4)}      # kept groups: 3 a + 2 b


@functools.lru_cache(maxsize=None)
def tiled_sheets(kept):
    """two_sheets tiled to `kept` kept groups: a block of 3 x a cells and, two layers above it, a block of 2 x b cells.  The two
    planes of every cell meet in the line x = -0.5 outside it: every group falls back."""
    a, b = SHEET_TILES[kept]
    M = _Mesh()
    V, T = _sheets(3, a, (0, 0, 0))
    M.t(T + M.v(V)[0])
    if b:
        V, T = _sheets(2, b, (0, 0, 2))
        M.t(T + M.v(V)[0])
    V, T = M.arrays()
    return _frozen(V, T, None, 1.0)


LANE_PATTERNS = {"lane_0": (0, 64, 128, 192), "lane_63": (63, 127, 191, 255), "only_64": (64,)}


@functools.lru_cache(maxsize=None)
def one_per_wave(pattern):
    """256 kept groups that do not fall back -- a flat sheet z = 0.25 over two rows of 128 cells, 2 x 2 vertices a cell: sorted
    positions 0 .. 255, one block of k_ts_place -- and, in the cells at the sorted positions of LANE_PATTERNS[pattern], one more
    member at z = 0.625 with a triangle of its own in the plane z = 0.625 + 0.25 (x - x_member), which meets the sheet 1.5 cells
    below the member's x: those groups fall back, exactly one per wave or one in all.  The far corners of such a triangle are
    groups of one vertex and one plane (rank 1, the minimiser is the vertex itself): they sort after the block and do not fall
    back."""
    M = _Mesh()
    i, j = np.meshgrid(np.arange(256), np.arange(4), indexing="xy")
    g = M.v(np.stack([0.5 * i.ravel() + 0.25, 0.5 * j.ravel() + 0.25, np.full(i.size, 0.25)], 1)).reshape(4, 256)
    a, b, c, d = g[:-1, :-1].ravel(), g[:-1, 1:].ravel(), g[1:, :-1].ravel(), g[1:, 1:].ravel()
    M.t(np.concatenate([np.stack([a, b, d], 1), np.stack([a, d, c], 1)]))
    for pos in LANE_PATTERNS[pattern]:
        x, y = pos % 128 + 0.5, pos // 128 + 0.5
        m = M.v([(x, y, 0.625), (x + 2, y, 1.125), (x, y + 2, 0.625)])
        M.t([tuple(m)])
    V, T = M.arrays()
    return _frozen(V, T, None, 1.0)


def _square_triangles(M, v, at, target):
    """Horizontal triangles (v, v + (s, 0, 0), v + (0, t, 0)) at the vertex v (M's index of the point `at`), s a power of two and t an
    integer, whose squared normals (s t)^2 are integers that add up to `target` exactly: greedily the largest square below what
    is left, its root cut to a multiple of s = the power of two below its square root, so that no edge is longer than 2^14."""
    left = int(target)
    while left:
        r = int(np.floor(np.sqrt(f64(left))))
        while r * r > left:
            r -= 1
        s = 1
        while s * s * 4 <= r:
            s *= 2
        t = r // s
        assert s <= 1 << 14 and t <= 1 << 14
        left -= (s * t) ** 2
        M.t([(v,) + tuple(M.v([(at[0] + s, at[1], at[2]), (at[0], at[1] + t, at[2])]))])


CENSUS_CELL = 0.25
U = CENSUS_CELL / 4                                 # the groups are drawn in units of a quarter cell
CUT = int(f64(1e-3) * f64(2.0 ** 62))               # 1e-3 (the binary64 value) times 2^62: an integer of 53 bits, exactly
CENSUS_FALLBACKS = ("zero_area", "zero_area", "zero_area", "high_face")   # (l0_small falls back only under the wrong l_max)


@functools.lru_cache(maxsize=None)
def census():
    """The fallback census, cell 1/4; coordinates below in units of U = 1/16, so that a cell is [4 k, 4 k + 4).  Every group lies
    in a cell of its own along x, y and z in [0, 4); positions are short binary fractions and every product and sum of these
    quadrics is exact in binary64, all normals are along an axis or come in pairs (n, n, 0), (-n, n, 0) whose products cancel,
    so A is diagonal exactly, the eigen-solve rotates nothing, and the results below are exact (asserted on the CPU).
      zero_area   x 0, 4, 8  three collinear vertices in three cells, one triangle: A = 0, l_max > 0 fails, all three fall back
      low_face    x 40  four members; the planes x + y = 42, x - y = 38 and z = 2 meet at (40, 2, 2), exactly ON the lower face
                        x = 40 of the cell [40, 44): inside, no fallback, the vertex is (40, 2, 2) U
      high_face   x 80  the same with x + y = 86 and x - y = 82: they meet at (84, 2, 2), exactly on the upper face: a fallback
      cut_exact   x 120 two members at z = 1 and 3; A = diag(2^62, 0, CUT): the third eigenvalue EQUALS 1e-3 l_max and takes no
                        part; the vertex keeps the centroid's z = 2 U
      cut_above   x 160 A = diag(2^62, 0, CUT + 1): one binary64 ulp above the cut: it takes part, and z moves to about 1 U
      l0_small    x 200 A = diag(0, 2^62, CUT + 1): l_max is not l_0
      unkept      x 240 (y 8) two members and a vertex of the next cell but one, collinear, in one triangle that is degenerate as groups:
                        A = 0 and it would fall back, but the group is not kept and not counted
    The strong plane of the cut groups is one triangle with edges 2^15 and 2^16 (n = 2^31); the third diagonal entry is a sum of
    squares of integers (_square_triangles) that are exact and add exactly.  -> the case and {name: the members' indices}."""
    M, at = _Mesh(), {}
    z = M.v(U * np.array([(1, 1, 1), (5, 1, 1), (9, 1, 1)], f64))
    M.t([tuple(z)])
    at["zero_area"] = z
    for name, x0, face in (("low_face", 40, 0), ("high_face", 80, 4)):
        px, inward = x0 + face, (1 if face == 0 else -1)
        pts = np.array([(px + inward * 1, 2 - inward * 1, 1), (px + inward * 1.5, 2 + inward * 1.5, 3)], f64)   # on x + y = px + 2; on x - y = px - 2
        m = M.v(U * pts)
        for v, p, (dx, dy, up) in zip(m, pts, ((1, -1, -16), (1, 1, 16))):                                     # (the far corners in cells of their own)
            M.t([(v,) + tuple(M.v(U * np.array([(p[0], p[1], p[2] + up), (p[0] + 16 * dx, p[1] + 16 * dy, p[2])], f64)))])
        for hx in (x0 + 2, x0 + 1):                                                                           # two members on the plane z = 2
            h = M.v(U * np.array([(hx, 2, 2), (hx + 16, 2, 2), (hx, 2 + 16, 2)], f64))
            M.t([tuple(h)])
            m = np.r_[m, h[0]]
        at[name] = m
    for name, x0, target, axis in (("cut_exact", 120, CUT, 0), ("cut_above", 160, CUT + 1, 0), ("l0_small", 200, CUT + 1, 1)):
        p = np.array([(x0 + 1) * U, U, U])
        m = M.v([p, p + (0, 0, 2 * U)])
        e1, e2 = ((0, 1 << 15, 0), (0, 0, 1 << 16)) if axis == 0 else ((0, 0, 1 << 16), (1 << 15, 0, 0))      # the strong plane: n = 2^31 along `axis`
        M.t([(m[0],) + tuple(M.v([p + e1, p + e2]))])
        _square_triangles(M, m[0], p, target - 9)
        M.t([(m[1],) + tuple(M.v([p + (3, 0, 2 * U), p + (0, 1, 2 * U)]))])                                    # the second member's one triangle: n = 3
        at[name] = m
    u = M.v(U * np.array([(241, 9, 1), (242, 9, 1), (249, 9, 1)], f64))
    M.t([tuple(u)])
    at["unkept"] = u
    V, T = M.arrays()
    return _frozen(V, T, None, CENSUS_CELL) + (at,)


# ---- H. magnitudes ------------------------------------------------------------------------------------------------------------------
SCALES = {"huge": 120, "tiny": -100, "subnormal": -140}


@functools.lru_cache(maxsize=None)
def scaled_corner(name):
    """tests/mesh_simplify_cases.corner (a finely cut box under a cell of 0.75: groups of rank 1, 2 and 3) times 2^120, 2^-100 and
    2^-140, the cell with it.  A power of two scales every binary64 product and sum of the quadric exactly, and none of them
    leaves the binary64 range (squared normals reach 2^(4 * 122) and 2^(4 * -143)), so every group takes the branch it takes
    unscaled: the minimiser with all three eigenpairs at the 8 corners, with two along the edges, with one on the faces; no
    fallback, and no l_max that is zero or not finite (a finite float32 mesh cannot make one but by zero areas: its squared
    normals lie between 2^-1192 and 2^1024).  At 2^-140 the coordinates are subnormal float32 values (the scaled decimals
    rounded onto multiples of 2^-149, so this is another mesh, not the scaled one), and so are the outputs."""
    V, T = corner()
    e = SCALES[name]
    return _frozen((V.astype(f64) * 2.0 ** e).astype(f32), T, None, float(f32(0.75 * 2.0 ** e)))
