"""The numpy restatement of the KdTree's shell walk (tests/points_cases.py: points_walk.h shell_walk and lb_sq, points_knn.h
walk_done) on the adversarial clouds of that module, on the CPU: its answers equal the brute-force models bit for bit on every
case, the boundary traps are what they claim to be (the walk without slack answers every one of them wrongly), the restated grid
arithmetic equals the host build of csrc/points_grid.h, and the candidate counts of every case are the recorded ones
(tests/golden/points_walk_cases.json, written by tools/gen_points_walk_cases.py).  tests/test_gpu_points_walk.py then holds the
device to the same rows and the same candidate counts."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import points_cases as PC
from tests import points_knn_model as KM
from tests import points_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "points_walk_cases.json")
f32 = np.float32


def _u(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_rows(got, want):
    for g, w in zip(got, want):
        assert g.shape == w.shape
        assert np.array_equal(_u(g), _u(w)) if w.dtype == f32 else np.array_equal(g, w)


@pytest.mark.parametrize("name", PC.NAMES)
def test_walk_equals_brute_force(name):
    """k = 1, 8 and 20 without a radius, k = 8 within a radius of about two cells, and everything within that radius."""
    P, Q = PC.case(name)
    r = PC.radius_of(name)
    assert np.isfinite(r) and r > 0
    idx, dist, found, cand, last = PC.answers(name, 1)
    bi, bd, _ = PM.nearest(P, Q)
    _same_rows((idx[:, 0], dist[:, 0], found), (bi, bd, (bi >= 0).astype(np.int32)))
    finite = np.isfinite(Q).all(axis=1)
    assert (cand[~finite] == 0).all() and (cand <= len(P)).all() and (cand[bi >= 0] >= 1).all()
    for k, md in ((8, np.inf), (20, np.inf), (8, r)):
        _same_rows(PC.answers(name, k, md)[:3], KM.knn(P, Q, k, md))
    _same_rows(PC.answers(name, None, r)[:3], KM.radius(P, Q, r))


@pytest.mark.parametrize("name", PC.NAMES)
def test_candidates_by_cell_ranges(name):
    """The walk model takes the points of shell r to be those whose cell lies at Chebyshev distance r; the header walks rows of
    cell ranges through the table of cell starts.  The two count the same candidates (every 7th query, and the last)."""
    _, Q = PC.case(name)
    W = PC.walk_of(name)
    _, _, _, cand, last = PC.answers(name, 8)
    for i in list(range(0, len(Q), 7)) + [len(Q) - 1]:
        if last[i] >= 0:
            assert W.candidates_by_ranges(Q[i], int(last[i])) == cand[i], (name, i)


@pytest.mark.parametrize("e", PC.TRAP_SCALES)
def test_traps_need_the_slack(e):
    """At least 8 traps per scale; the walk finds the lone point beyond the boundary of every one of them, and the walk with both
    slack terms zeroed stops a shell early on every one of them, at the second point."""
    name = f"traps_{e}"
    P, Q = PC.case(name)
    n, winners = PC.trap_queries(name)
    assert n >= 8
    assert np.array_equal(PM.nearest(P, Q[:n])[0], winners)
    idx, _, _, _, last = PC.answers(name, 1)
    assert np.array_equal(idx[:n, 0], winners) and (last[:n] >= 1).all()
    bare, _, _, _, bare_last = PC.walk_of(name).many(Q[:n], 1, slack=False)
    print(name, n, "traps; without slack:", int((bare[:, 0] != winners).sum()), "wrong, last shells", bare_last.tolist())
    assert (bare[:, 0] != winners).all() and (bare[:, 0] >= 0).all() and (bare_last == 0).all()
    # the same traps at every scale: the construction scales exactly
    P0, Q0 = PC.case("traps_0")
    assert np.array_equal(_u(P), _u(PC.scaled(P0, e))) and np.array_equal(_u(Q), _u(PC.scaled(Q0, e)))


@pytest.mark.parametrize("e", [-40, 40])
def test_powers_of_two_scale_exactly(e):
    """The base cloud and its queries times 2^e: the same indices, every distance exactly 2^e times scale 1's, the same candidates.
    (Not beyond: at 2^60 the d2 of the 42 queries at 1000 and 10^6 extents overflows, so they find nothing; at 2^-62 the indices and
    candidates still agree but d2 is denormal and 2^-124 d2 rounds -- the scale_<e> cases go on from there against brute force.)"""
    B, BQ = PC.case("base")
    ref = PC.answers("base", 8)
    idx, dist, found, cand, last = PC.Walk(PC.scaled(B, e)).many(PC.scaled(BQ, e), 8)
    assert (ref[2] == 8).all()
    assert np.array_equal(idx, ref[0]) and np.array_equal(_u(dist), _u(PC.scaled(ref[1], e)))
    assert np.array_equal(found, ref[2]) and np.array_equal(cand, ref[3]) and np.array_equal(last, ref[4])


def test_denormal_scales_are_what_they_claim():
    """What the scale cases are for, on the brute-force model: at 2^-70 some nearest indices differ from scale 1's (d2 is denormal),
    at 2^-75 and 2^-140 most d2 are 0, at 2^100 only a query equal to a static point finds anything, at 2^64 some queries do and some
    do not."""
    B, BQ = PC.case("base")
    i0 = PM.nearest(B, BQ)[0]
    near = PC.near_queries("base")

    def nearest_of(e):
        P, Q = PC.case(f"scale_{e}")
        return PM.nearest(P, Q)

    assert (nearest_of(-70)[0] != i0).any()
    for e in (-75, -140):
        assert (nearest_of(e)[1][near] == 0).mean() > 0.5
    i100, d100, _ = nearest_of(100)
    assert ((i100 >= 0) == (d100 == 0)).all() and 0 < (i100 >= 0).sum() <= PC.N_NEAR
    i64 = nearest_of(64)[0]
    assert (i64 >= 0).any() and (i64 < 0).any()
    assert PC.walk_of("scale_-140").G["inv_h"] == np.inf and PC.walk_of("scale_-140").G["slack"] == 0


@pytest.fixture(scope="module")
def grid_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("points_grid_host")
    exe = str(d / "points_grid_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "points_grid_host.cpp"), "-o", exe])

    def cells(lo, hi, n, X):
        X = np.ascontiguousarray(X, f32).reshape(-1, 3)
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            f.write(np.asarray(lo, f32).tobytes() + np.asarray(hi, f32).tobytes() + np.array([n, len(X)], np.int64).tobytes() + X.tobytes())
        p = subprocess.run([exe, "cells", src, dst], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and "cells ok" in p.stdout, p.stdout[-1000:] + p.stderr[-1000:]
        raw = open(dst, "rb").read()
        return np.frombuffer(raw[:12], np.int32), np.frombuffer(raw[12:24], f32), np.frombuffer(raw[24:], np.int32).reshape(-1, 3)
    return cells


@pytest.mark.parametrize("name", PC.NAMES)
def test_restated_grid_equals_points_grid_h(grid_host, name):
    """dim, h, inv_h, slack and the cell of every point and query of the case, and of a NaN, both infinities and +-FLT_MAX along
    every axis: the numpy restatement (tests/meshsdf_cases.py) against points_grid.h built for the host, bit for bit."""
    P, Q = PC.case(name)
    G = PC.cloud_grid(P)
    odd = np.array([[v, P[0, 1], P[0, 2]] for v in (np.nan, np.inf, -np.inf, PC.FLT_MAX, -PC.FLT_MAX)], f32)
    X = np.concatenate([P, Q, odd, odd[:, [1, 0, 2]], odd[:, [2, 1, 0]]])
    dim, hs, cells = grid_host(P.min(0), P.max(0), len(P), X)
    assert tuple(dim) == tuple(G["dim"])
    assert np.array_equal(_u(hs), _u(np.array([G["h"], G["inv_h"], G["slack"]], f32))), (hs, G)
    mine = PC.cell_of(G, X)
    assert np.array_equal(mine, cells), (name, np.nonzero((mine != cells).any(axis=1))[0][:5])
    if name == "scale_-140":      # (x - lo) * inv_h is 0 * inf at x = lo: fmaxf sends that NaN to cell 0, every other point to the last cell
        pc = cells[:len(P)]
        assert G["inv_h"] == np.inf and ((pc == 0) | (pc == np.array(G["dim"]) - 1)).all() and (pc == 0).any()
    assert (cells[len(P) + len(Q)] == [0, cells[0, 1], cells[0, 2]]).all()      # the NaN


def test_candidate_counts_are_the_recorded_ones():
    """tools/gen_points_walk_cases.py, run again: sizes, grids, candidates and last shells of every case."""
    with open(GOLDEN) as f:
        recorded = json.load(f)
    assert PC.summary() == recorded
