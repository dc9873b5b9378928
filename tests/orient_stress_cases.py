"""The clouds of the orientation stress tests (tests/test_orient_stress_cases.py on the CPU, tests/test_gpu_orient_stress.py on the
device): inputs that sit on the decisions of csrc/points_orient.h and on the schedule of csrc/lib_orient.hip, which the clouds of
tests/orient_cases.py only cross by chance.  Not a test module.

Every case is a dict: P (n, 3) float32, normals (n, 3) float32, k, max_distance, max_seeds, and rows -- (index (n, k) int32,
found (n,) int32), the k-nearest rows in closed form where the brute force of tests/points_knn_model.py cannot run (the long lines),
else None.  All are made once and read-only; tests/orient_model.orient is the yardstick of every one.
"""
import functools
import os
import re

import numpy as np

from tests import orient_cases as OC
from tests import orient_model as OM

f32, f64 = np.float32, np.float64
INF = np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIP = 2048 * 256            # the lanes of one trip of k_or_seed_find: at most 2048 blocks of 256 (csrc/lib_orient.hip)
LINE = TRIP + 40             # the long lines: 40 points into the second trip


def batch():
    """kBatch of csrc/lib_orient.hip: the rounds queued between two reads of the control block, read from the source."""
    with open(os.path.join(ROOT, "sdfkit_amd", "csrc", "lib_orient.hip")) as f:
        return int(re.search(r"constexpr int kBatch = (\d+);", f.read()).group(1))


def seed_grid():
    """The cap on the blocks of k_or_seed_find and its block size, read from the source: -> lanes of one trip."""
    src = os.path.join(ROOT, "sdfkit_amd", "csrc")
    with open(os.path.join(src, "lib_orient.hip")) as f:
        cap = int(re.search(r"k_or_seed_find, dim3\(\(unsigned\)grid_for\(\(size_t\)n, kBlock, (\d+)\)\)", f.read()).group(1))
    with open(os.path.join(src, "points_walk.h")) as f:
        block = int(re.search(r"constexpr int kBlock = (\d+);", f.read()).group(1))
    return cap * block


def case(P, normals, k, max_distance=INF, max_seeds=64, rows=None):
    c = {"P": np.ascontiguousarray(P, f32), "normals": np.ascontiguousarray(normals, f32), "k": int(k), "max_distance": max_distance,
         "max_seeds": int(max_seeds), "rows": rows}
    for a in (c["P"], c["normals"]) + (tuple(rows) if rows is not None else ()):
        a.setflags(write=False)
    return c


def model(c):
    """The model's answer to a case -> (normals, stats)."""
    return OM.orient(c["P"], c["normals"], c["k"], c["max_distance"], c["max_seeds"], rows=c["rows"])


def window_rows(P, k, window, spacing2):
    """The exact k-nearest rows of a cloud whose point i has every point outside i - window .. i + window at a d2 of at least
    `spacing2` (the caller's knowledge of its cloud), by the contract's formula: float32 d2 = (dx*dx + dy*dy) + dz*dz, ascending by
    (d2, index).  Asserts that the k-th d2 found is below spacing2, so that no point outside the window belongs to a row."""
    P = np.asarray(P, f32)
    n = len(P)
    j = np.arange(n)[:, None] + np.arange(-window, window + 1)[None, :]
    ok = (j >= 0) & (j < n)
    Q = P[np.clip(j, 0, n - 1)]
    d = P[:, None, :] - Q
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == f32
    d2 = np.where(ok, d2, f32(np.inf))
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]          # (the candidates ascend in index: stable = ties to the lower)
    kth = np.take_along_axis(d2, order[:, -1:], axis=1)[:, 0]
    assert (kth < f32(spacing2)).all()
    return np.take_along_axis(j, order, axis=1).astype(np.int32), np.full(n, k, np.int32)


def _tilted(rs, count):
    """Unit normals within about 25 degrees of +-z, the sign at random."""
    v = np.concatenate([0.25 * rs.standard_normal((count, 2)), np.ones((count, 1))], axis=1)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * rs.choice([-1.0, 1.0], (count, 1))).astype(f32)


# ---- 1. the seed search past one trip ----
LINE_VALID = (np.arange(100, 120), np.arange(LINE - 30, LINE))


@functools.lru_cache(maxsize=None)
def line():
    """LINE points at (0, 0, i); valid normals at 100 .. 119 and at the last 30 only: the first seed is the last point, in the
    second trip of the seed search, the second seed index 119."""
    rs = np.random.default_rng(71)
    P = np.zeros((LINE, 3), f32)
    P[:, 2] = np.arange(LINE, dtype=f32)
    assert np.array_equal(P[:, 2].astype(np.int64), np.arange(LINE))           # exact in float32
    Nn = np.zeros((LINE, 3), f32)
    for idx in LINE_VALID:
        Nn[idx] = _tilted(rs, len(idx))
    return case(P, Nn, 3, rows=line_rows(LINE))


def line_rows(n):
    """[i, i - 1, i + 1] (the tie in d2 goes to the lower index); the ends: [0, 1, 2] and [n - 1, n - 2, n - 3]."""
    i = np.arange(n, dtype=np.int32)
    idx = np.stack([i, i - 1, i + 1], axis=1)
    idx[0] = [0, 1, 2]
    idx[-1] = [n - 1, n - 2, n - 3]
    return idx, np.full(n, 3, np.int32)


TIE_LOW, TIE_HIGH = 1000, TRIP + 12


@functools.lru_cache(maxsize=None)
def tie_across_trips():
    """LINE points at (i, 0, 0), two of them lifted to the same z = 0.25: TIE_LOW in the first trip of the seed search, TIE_HIGH in
    the second.  Valid normals, all pointing down, at those two and their three neighbours on either side; ONE seed is allowed, so
    the output shows which of the two was taken: the one of lower index."""
    P = np.zeros((LINE, 3), f32)
    P[:, 0] = np.arange(LINE, dtype=f32)
    P[[TIE_LOW, TIE_HIGH], 2] = 0.25
    Nn = np.zeros((LINE, 3), f32)
    for t in (TIE_LOW, TIE_HIGH):
        Nn[t - 3:t + 4] = [0.0, 0.0, -1.0]
    return case(P, Nn, 3, max_seeds=1, rows=window_rows(P, 3, 3, 16.0))


def sample_indices(n, count=1000, seed=72):
    """About `count` indices of a long line: both ends, the indices around the end of the first trip and around the valid normals,
    the rest at random."""
    rs = np.random.default_rng(seed)
    fixed = np.concatenate([np.arange(0, 8), np.arange(n - 8, n), np.arange(TRIP - 4, TRIP + 4), np.arange(96, 124), np.arange(n - 34, n),
                            np.arange(TIE_LOW - 5, TIE_LOW + 6), np.arange(TIE_HIGH - 5, TIE_HIGH + 6)])
    return np.unique(np.concatenate([fixed, rs.integers(0, n, count - len(fixed))]))


# ---- 2. the deciding launch at a batch edge ----
def ladder(stations, seed=73):
    """A ladder: points (x, 0, -x / 512) and (x, 0.25, -x / 512), x = 0 .. stations - 1, normals +-(0, 0, 1).  With k = 3 a row is the
    point, its partner and the point one station up (the tie with the one below goes to the lower index), so the growth takes one
    station per round from the seed, index 0."""
    rs = np.random.default_rng(seed + stations)
    x = np.repeat(np.arange(stations, dtype=f64), 2)
    P = np.stack([x, np.tile([0.0, 0.25], stations), -x / 512.0], axis=1).astype(f32)
    assert np.array_equal(P.astype(f64)[:, 2], -x / 512.0)
    Nn = np.zeros((2 * stations, 3), f32)
    Nn[:, 2] = rs.choice([-1.0, 1.0], 2 * stations)
    return case(P, Nn, 3)


@functools.lru_cache(maxsize=None)
def ladders_at_batch_edges(batches=(1, 2)):
    """-> {(b, d): ladder}: the ladder whose first launch to find the growth over -- launch number rounds + 1, the seed being
    launch 1 and `rounds` the model's (seed and live rounds) -- is the last launch of batch b (number 1 + b * kBatch) plus d, for
    d = -1, 0, 1, 2: the last but one of the batch, the last, and the first and second of the next."""
    B = batch()
    want = {1 + b * B + d: (b, d) for b in batches for d in (-1, 0, 1, 2)}
    out = {}
    for stations in range(2, (max(batches) + 1) * B):
        c = ladder(stations)
        rounds = model(c)[1]["rounds"]
        if rounds + 1 in want and want[rounds + 1] not in out:
            out[want[rounds + 1]] = c
    assert len(out) == len(want)
    return out


# ---- 3. weights on the level thresholds ----
def threshold_dots():
    """The dots of the chain, in the order of the chain: each threshold, the float32 next below it, the least subnormal, both
    zeros, and the negatives -- descending in magnitude, so that the links of level l follow those of level l - 1."""
    below = lambda t: np.nextafter(f32(t), f32(0))
    mags = [f32(1), below(1)]
    for t in (0.9375, 0.75, 0.5):
        mags += [f32(t), below(t)]
    mags.append(f32(2.0 ** -149))
    c = []
    for m in mags:
        c += [m, -m]
    return np.array(c + [f32(0.0), f32(-0.0)], f32)


@functools.lru_cache(maxsize=None)
def threshold_chain():
    """Points (0, 0, -i) with k = 2: the row of i is [i, i - 1] (the tie with i + 1 goes to the lower index), so the growth runs down
    the chain from the seed, index 0, one link per round.  The normals alternate between (1, 0, 0) and (c, 1, 0): the dot of a link
    is c exactly, and every c makes two links, into its point and out of it."""
    c = threshold_dots()
    n = 2 * len(c) + 1
    P = np.zeros((n, 3), f32)
    P[:, 2] = -np.arange(n, dtype=f32)
    Nn = np.zeros((n, 3), f32)
    Nn[0::2] = [1.0, 0.0, 0.0]
    Nn[1::2, 0] = c
    Nn[1::2, 1] = 1.0
    return case(P, Nn, 2)


# ---- 4. two sources of equal weight and opposite sign ----
def equal_weights(exchanged):
    """A seed S on top, two sources A and B below it at the same height, the target T below them at the same d2 from both: T's row
    is [T, the lower index of A and B, the higher], and dot(T, A) = 0.5 = -dot(T, B).  exchanged: B takes the lower index."""
    S, A, B, T = (0, 0, 2), (-1, 0, 1), (1, 0, 1), (0, 0, 0)
    nS, nA, nB, nT = (0, 0, 1), (0.5, 0, 1), (-0.5, 0, 1), (1, 0, 0)
    P = [S, B, A, T] if exchanged else [S, A, B, T]
    Nn = [nS, nB, nA, nT] if exchanged else [nS, nA, nB, nT]
    return case(np.array(P, f32), np.array(Nn, f32), 3)


# ---- 5. small edges ----
BAD = np.array([[0, 0, 0], [-0.0, 0, -0.0], [np.nan, 0, 1], [0, np.inf, 0], [1, 0, -np.inf]], f32)


@functools.lru_cache(maxsize=None)
def no_valid_normal(valid_at=None):
    """50 random points whose normals are all zero or not finite; valid_at: that one gets (0.6, 0, -0.8)."""
    rs = np.random.default_rng(74)
    P = rs.random((50, 3), dtype=f32)
    Nn = BAD[rs.integers(0, len(BAD), 50)].copy()
    if valid_at is not None:
        Nn[valid_at] = [0.6, 0.0, -0.8]
    return case(P, Nn, 8)


# seed normals with n_z == 0 (either zero), one per branch of seed_sign: |n_x| > |n_y|, <, ==, each with both signs of the winner
SEED_NORMALS = np.array([[0.75, 0.5, 0], [-0.75, 0.5, 0], [0.5, -0.75, 0], [0.5, 0.75, 0], [-0.5, -0.75, -0.0], [0.5, -0.5, 0], [-0.5, 0.5, 0],
                         [-0.5, -0.5, 0], [0.5, 0.5, -0.0], [0, -1, 0], [-0.0, 1, 0], [-1, 0, -0.0], [-1, -0.0, 0]], f32)


def flat_seed(normal):
    """Three points, the top one the seed with `normal`, the others with the same normal: they take the seed's sign."""
    P = np.array([[0, 0, 1], [1, 0, 0.5], [2, 0, 0]], f32)
    return case(P, np.tile(np.asarray(normal, f32), (3, 1)), 2)


def zero_z_ties(max_seeds):
    """Twelve points a unit apart in a plane whose z mix -0 and +0 (index 0: -0), each alone within max_distance, the normals all
    down: every seed orients itself only, and the seeds come in index order, -0 equal to +0."""
    P = np.zeros((12, 3), f32)
    P[:, 0] = np.arange(12)
    P[[0, 3, 4, 7, 10], 2] = -0.0
    Nn = np.tile(np.array([[0.0, 0.0, -1.0]], f32), (12, 1))
    return case(P, Nn, 4, max_distance=f32(0.25), max_seeds=max_seeds)


# ---- 6. max_distance = 0 ----
def triples(max_seeds):
    """100 distinct points held three times each, in random order, random unit normals: with max_distance = 0 a row is the three
    holders of a point, so every distinct point needs a seed of its own."""
    rs = np.random.default_rng(75)
    D = rs.random((100, 3), dtype=f32)
    assert len(np.unique(D, axis=0)) == 100
    P = np.repeat(D, 3, axis=0)[rs.permutation(300)]
    v = rs.standard_normal((300, 3))
    return case(P, (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32), 8, max_distance=f32(0.0), max_seeds=max_seeds)


# ---- 7. scaled clouds ----
SCALES = (-70, 40)


def scaled_sphere(e):
    """The sphere of tests/orient_cases.py times 2^e (exact), with the unscaled cloud's unoriented normals."""
    P, _, nrm = OC.cloud("sphere")
    S = (P * f32(2.0 ** e)).astype(f32)
    assert np.array_equal(S.astype(f64), P.astype(f64) * 2.0 ** e)
    return case(S, nrm, 8)
