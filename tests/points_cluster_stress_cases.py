"""The clouds of the clustering stress tests (tests/test_points_cluster_stress_cases.py on the CPU, tests/test_gpu_points_cluster_stress.py
on the device): inputs that the shuffled clouds of tests/points_cluster_cases.py never give KdTree.Clusters / SelectClusters --
chains whose index order decides the depth of the forest and the number of hook rounds, a border point between six clusters with
six candidates at one d2, waves whose lanes are laid out by index for the sizes kernel, point counts on the edges of the scan's
blocks and beyond its 256 block totals, and clumps whose squared distances overflow or underflow binary32.  Not a test module.

Every cloud is (n, 3) float32 and is generated in closed form or from a seeded np.random.default_rng, so it is the same bits on
every machine.  The numpy model (tests/points_cluster_model.py) is the yardstick of every one; where a cloud is too large for the
model's brute-force neighbour rows, the rows are given here in closed form and proved on the small versions."""
import functools

import numpy as np

f32, f64, i32, i64 = np.float32, np.float64, np.int32, np.int64
INF = np.inf


def _frozen(P):
    P = np.ascontiguousarray(P, f32)
    P.setflags(write=False)
    return P


def _exact(P64):
    """The binary64 coordinates as float32, which must hold them exactly."""
    P = np.asarray(P64, f64).astype(f32)
    assert np.array_equal(P.astype(f64), P64), "a coordinate is not exact in binary32"
    return _frozen(P)


# ---- 1. chains ------------------------------------------------------------------------------------------------------------------
CHAIN_N = 1 << 14
CHAIN_ORDERS = ("ascending", "descending", "bit_reversed")


def bit_reversed(n):
    """The permutation x -> x with its log2(n) bits reversed (n a power of two); its own inverse."""
    bits = int(n).bit_length() - 1
    assert 1 << bits == n
    x = np.arange(n, dtype=i64)
    out = np.zeros(n, i64)
    for b in range(bits):
        out |= ((x >> b) & 1) << (bits - 1 - b)
    return out


def chain_order(name, n):
    """index_of[x]: the index of the point at x."""
    x = np.arange(n, dtype=i64)
    if name == "bit_reversed":
        return bit_reversed(n)
    return {"ascending": x, "descending": n - 1 - x}[name]


@functools.lru_cache(maxsize=None)
def chain(name, n=CHAIN_N):
    """n points at x = 0 .. n - 1, y = z = 0; the point at x has index chain_order(name, n)[x].  At radius 1 the clusters' graph is
    a path.  Hooked from a snapshot, the two sorted orders leave parent[i] = i - 1, a tree of depth n - 1; the bit-reversed order
    needs the most hook rounds a path can need, ceil(log2 n) + 1."""
    index_of = chain_order(name, n)
    P = np.zeros((n, 3), f64)
    P[index_of, 0] = np.arange(n)
    return _exact(P)


def chain_rows(P):
    """CM.neighbours(P, 1.0) of a chain in closed form: the point at x sees x - 1, x and x + 1, ordered by (d2, index) -- itself,
    then the one or two at d2 = 1 by ascending index.  -> (offsets (n + 1,) int64, index int32)."""
    x = P[:, 0].astype(i64)
    n = len(x)
    index_of = np.empty(n, i64)
    index_of[x] = np.arange(n)
    big = n                                                     # (an index no point has: sorts last, then dropped)
    left = np.where(x > 0, index_of[np.maximum(x - 1, 0)], big)
    right = np.where(x < n - 1, index_of[np.minimum(x + 1, n - 1)], big)
    row = np.stack([np.arange(n), np.minimum(left, right), np.maximum(left, right)], axis=1)
    keep = row < big
    off = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(i64)
    return off, row[keep].astype(i32)


def chain_expected(P, min_points):
    """What CM.cluster gives on a chain at radius 1 and min_points 1 .. 3, in closed form: one cluster of all; the two ends count 2
    and are border points at min_points = 3."""
    x = P[:, 0].astype(i64)
    n = len(x)
    assert 1 <= min_points <= 3 and n >= 3
    counts = np.where((x == 0) | (x == n - 1), 2, 3).astype(i32)
    core = counts >= min_points
    ncore = int(core.sum())
    return {"labels": np.zeros(n, i32), "sizes": np.array([n], i32), "core": core, "counts": counts, "n_clusters": 1, "stats": [1, ncore, n - ncore, 0]}


# ---- 2. the six-armed star------------------------------------------------------------------------------------------------------
STAR_DIRECTIONS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f64)
STAR_ARM = 16                                    # points per arm, at distances 1 + k / 16 from the centre
STAR_MIN_POINTS = 8
_STAR_BASE = (0, 3, 5, 1, 4, 2)
STAR_PERMUTATIONS = tuple(_STAR_BASE[r:] + _STAR_BASE[:r] for r in range(6))     # every arm is first once
STAR_CENTRES = ("first", "middle", "last")
STAR_FRAMES = ((1.0, (0.0, 0.0, 0.0)), (2.0 ** -20, (0.0, 0.0, 0.0)), (4.0, (37.25, -11.5, 3.0625)), (2.0 ** 10, (2.0 ** 14, 2.0 ** 14, -2.0 ** 14)))
STAR_LAYOUTS = tuple((p, c, f) for p in range(len(STAR_PERMUTATIONS)) for c in STAR_CENTRES for f in range(len(STAR_FRAMES)))


@functools.lru_cache(maxsize=None)
def star(perm, centre, frame):
    """-> (points (97, 3), radius, centre index, inner (6,): the index of the inner point of arm a).  Six arms of 16 points along
    +-x, +-y, +-z at distances (1 + k / 16) * scale from the centre point, k = 0 .. 15, radius = scale, min_points = 8: every arm
    point is core (16 or 17 within the radius), every arm its own cluster (two arms are sqrt(2) * scale apart at the least), and
    the centre has 7 within the radius: border, with the six inner points (k = 0) as core candidates at d2 = scale^2 exactly.
    Index order: the outer points of arm 0, outermost first, then those of arm 1 .. 5 -- so cluster a is arm a --, then the six
    inner points in the order STAR_PERMUTATIONS[perm] of their arms; the centre is put first, in the middle or last.  The centre
    follows the inner point of the lowest index: arm STAR_PERMUTATIONS[perm][0], which is not cluster 0 in most orders."""
    scale, offset = STAR_FRAMES[frame]
    order = STAR_PERMUTATIONS[perm]
    arm_of = [a for a in range(6) for _ in range(STAR_ARM - 1)] + list(order)
    k_of = [k for _ in range(6) for k in range(STAR_ARM - 1, 0, -1)] + [0] * 6
    at = {"first": 0, "middle": len(arm_of) // 2, "last": len(arm_of)}[centre]
    arm_of.insert(at, -1)
    k_of.insert(at, 0)
    arm_of, k_of = np.array(arm_of), np.array(k_of, f64)
    P = np.where((arm_of >= 0)[:, None], STAR_DIRECTIONS[arm_of] * ((1 + k_of / STAR_ARM) * scale)[:, None], 0.0) + np.array(offset, f64)
    inner = np.array([int(np.flatnonzero((arm_of == a) & (k_of == 0))[0]) for a in range(6)])
    return _exact(P), float(scale), at, inner


# ---- 3. waves laid out by index --------------------------------------------------------------------------------------------------
WAVES_RADIUS, WAVES_MIN_POINTS = 1.0, 4          # (a border point needs itself and a core point within the radius: min_points >= 3;
#                                                    4 leaves room for one more neighbour that is not core)
A, B, C_, D, NOISE = 0, 1, 2, 3, -1
WAVES = (
    [A] * 64,                                    # one cluster
    [NOISE] + [A] * 63,                          # noise at lane 0, the rest one cluster
    [A, NOISE] * 32,                             # one cluster and noise alternating
    [NOISE] * 64,                                # noise only
    [A] * 32 + [B] * 32,                         # two clusters, split inside the wave
    [B] * 63 + [C_],                             # a third cluster at lane 63 only
    [C_] * 64,                                   # one cluster, four of its lanes border points
    [D] * 37,                                    # the last, partial wave
)
WAVES_BORDER_LANES = (5, 20, 41, 63)             # of wave 6
WAVES_LABELS = np.array([c for w in WAVES for c in w], i32)
WAVES_N = 485


@functools.lru_cache(maxsize=None)
def waves():
    """-> (points (485, 3), border (485,) bool).  Clusters A .. D are clumps on the x axis, 100 apart, their core members 1 / 512
    apart (every two of a clump within the radius 1); the noise points are 4 apart on a line far from all of them.  The four
    border points of C are at distance exactly 1 from C's first core member only (in +-y and +-z; any other member is farther by
    an ulp at the least), so they have 2 within the radius -- and the first of them 3: one noise point sits 0.5 beyond it, within
    its radius, nearer to it than its core point and itself out of reach of any core point.  Indices: in the order of WAVES."""
    assert len(WAVES_LABELS) == WAVES_N
    border = np.zeros(WAVES_N, bool)
    border[6 * 64 + np.array(WAVES_BORDER_LANES)] = True
    P = np.zeros((WAVES_N, 3), f64)
    seen = {A: 0, B: 0, C_: 0, D: 0, NOISE: 0}
    spots = [(0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    nb = 0
    for i, c in enumerate(WAVES_LABELS.tolist()):
        if border[i]:
            P[i] = np.array([100.0 * C_, 0, 0]) + spots[nb]
            nb += 1
            continue
        j = seen[c]
        seen[c] += 1
        if c == NOISE:
            P[i] = (0, 1000 + 4 * j, 0) if j != 40 else (100.0 * C_, 1.5, 0)      # (the one beyond C's first border point)
        else:
            P[i] = (100.0 * c + j / 512, 0, 0)
    return _exact(P), border


# ---- 5. isolated pairs -----------------------------------------------------------------------------------------------------------
PAIRS_RADIUS = 0.5
PAIRS_MODEL_N = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)     # the edges of a wave, a block and the scan's 2048
PAIRS_LARGE_N = 256 * 2048 + 2                   # 257 scan blocks: k_scan_sums goes round its loop twice and carries


@functools.lru_cache(maxsize=None)
def pairs(n):
    """Point i at (i // 2 mod 1024, i // 2 // 1024, 0.25 * (i mod 2)): pairs 0.25 apart, 1 from every other pair at the least."""
    i = np.arange(n, dtype=i64)
    return _exact(np.stack([(i // 2) % 1024, (i // 2) // 1024, 0.25 * (i % 2)], axis=1).astype(f64))


def pairs_rows(n):
    """CM.neighbours(pairs(n), 0.5) in closed form: itself, then its partner i ^ 1 where that exists."""
    i = np.arange(n, dtype=i64)
    row = np.stack([i, i ^ 1], axis=1)
    keep = row < n
    return np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(i64), row[keep].astype(i32)


def pairs_expected(n, min_points):
    """What CM.cluster gives on pairs(n) at radius 0.5, in closed form."""
    i = np.arange(n, dtype=i64)
    counts = np.where((i ^ 1) < n, 2, 1).astype(i32)
    core = counts >= min_points
    labels = np.where(core, i // 2, -1).astype(i32) if min_points <= 2 else np.full(n, -1, i32)
    if min_points == 2 and n % 2:                # (the last point alone is noise, and so the last cluster is not there)
        labels[-1] = -1
    nc = 0 if min_points > 2 else (n + 1) // 2 if min_points == 1 else n // 2
    sizes = np.full(nc, 2, i32)
    if min_points == 1 and n % 2:
        sizes[-1] = 1
    ncore = int(core.sum())
    return {"labels": labels, "sizes": sizes, "core": core, "counts": counts, "n_clusters": nc, "stats": [nc, ncore, 0, n - ncore]}


def pairs_keep(n_clusters):
    return (np.arange(n_clusters) % 3 != 1).astype(np.uint8)


def pairs_kept(n):
    """The indices SelectClusters keeps of pairs(n)'s labels at min_points = 1 under pairs_keep, in closed form."""
    i = np.arange(n, dtype=i64)
    return i[(i // 2) % 3 != 1].astype(i32)


# ---- 6. d2 beyond binary32 -------------------------------------------------------------------------------------------------------
OVERFLOW_CASES = ((INF, 1, [2, 80, 0, 0]), (3e38, 1, [2, 80, 0, 0]), (INF, 41, [0, 0, 0, 80]))          # (radius, min_points, stats)
UNDERFLOW_CASES = ((0.0, 1, [51, 100, 0, 0]), (1e-45, 1, [51, 100, 0, 0]))


@functools.lru_cache(maxsize=None)
def overflow():
    """-> (points (80, 3), clump (80,) int).  Two clumps of 40 points, of extent 1e18, around +2e19 and -2e19 on every axis,
    shuffled: within a clump d2 is below 3e36; between them every squared difference is 1.4e39 at the least, beyond FLT_MAX, so d2
    is +inf and the two are no neighbours at any radius, +inf included."""
    rng = np.random.default_rng([0x636C7573, 6, 1])
    clump = np.repeat([0, 1], 40)
    P = np.where(clump[:, None] == 0, 2e19, -2e19) + rng.uniform(-5e17, 5e17, (80, 3))
    order = rng.permutation(80)
    return _frozen(P[order].astype(f32)), clump[order]


@functools.lru_cache(maxsize=None)
def underflow():
    """-> (points (100, 3), tiny (100,) bool).  50 points of scale 1e-24, pairwise distinct, whose every d2 (1e-48) underflows to 0:
    duplicates of each other at radius 0; and 50 of scale 1e-18, whose d2 (1e-36) is an ordinary float32: each its own cluster."""
    rng = np.random.default_rng([0x636C7573, 6, 2])
    tiny = np.repeat([True, False], 50)
    P = rng.uniform(-1, 1, (100, 3)) * np.where(tiny, 1e-24, 1e-18)[:, None]
    order = rng.permutation(100)
    return _frozen(P[order].astype(f32)), tiny[order]
