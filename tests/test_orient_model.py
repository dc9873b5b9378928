"""CPU checks of the consistent orientation of normals: the numpy model (tests/orient_model.py) on the recorded clouds
(tests/orient_cases.py, tests/golden/orient_cases.json), the shared decisions of the kernels (sdfkit_amd/csrc/points_orient.h) built
with g++ against the model, and the two new C-ABI entry points: exported, and refusing to run without a device."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sdfkit_amd import _native as N
from tests import orient_cases as OC
from tests import orient_model as OM

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "orient_cases.json")
ENTRY_POINTS = ["sdfk_points_orient_normals", "sdfk_points_orient_normals_device"]


@pytest.fixture(scope="module")
def records():
    return OC.records()


# ---- the model on the recorded clouds ----
def test_recorded_cases_are_the_models(records):
    with open(GOLDEN) as f:
        assert json.load(f) == records


def test_unoriented_normals_are_half_wrong(records):
    """The gap: without a viewpoint about half of the normals of a closed surface point inward."""
    for name in ("sphere", "torus", "two_spheres", "cube", "plate"):
        assert 0.4 < records[name]["before"] < 0.6, name


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_smooth_closed_surfaces_come_out_entirely_outward(records, name):
    assert records[name]["after"] == 1.0
    assert records[name]["seeds"] == (2 if name == "two_spheres" else 1)


@pytest.mark.parametrize("name", ["cube", "plate"])
def test_sharp_and_thin_surfaces_are_right_to_a_percent(records, name):
    assert records[name]["after"] >= 0.99 and records[name + "_single_level"]["after"] >= 0.99
    assert sum(1 for c in records[name]["levels"] if c) >= 2                      # the thresholds are exercised
    assert records[name]["after"] >= records[name + "_single_level"]["after"]     # what the levels buy, never a loss here


def test_strip_takes_about_its_length_in_rounds(records):
    r = records["strip"]
    assert r["after"] == 1.0 and r["rounds"] > 300 and r["seeds"] == 1


def test_model_on_hand_made_cases():
    # a row of four points along x, normals +-z: one seed (the highest point, index 2), everything agrees with it
    P = np.array([[0, 0, 0], [1, 0, 0.1], [2, 0, 0.2], [3, 0, 0.1]], f32)
    Nn = np.array([[0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, -1]], f32)
    # (k = 3: every row holds point 2 or a neighbour of it; one round orients all, then one empty round per level)
    out, st = OM.orient(P, Nn, 3)
    assert (out[:, 2] == 1).all() and st == {"rounds": 6, "seeds": 1, "flipped": 3, "unreached": 0, "invalid": 0, "levels": [3, 0, 0, 0]}
    # the same with an invalid normal in the middle: it is no bridge (k = 2: each row is the point and one neighbour)
    Nn[1] = 0
    out, st = OM.orient(P, Nn, 2)
    assert st["invalid"] == 1 and st["seeds"] == 2 and np.array_equal(out[1].view(np.uint32), Nn[1].view(np.uint32))
    assert (out[[0, 2, 3], 2] == 1).all()
    # max_seeds = 1 leaves point 0 unreached and untouched
    out, st = OM.orient(P, Nn, 2, max_seeds=1)
    assert st["unreached"] == 1 and st["seeds"] == 1 and out[0, 2] == -1
    # perpendicular normals: a dot of exactly 0 is accepted at the last level only and keeps the normal as it is
    P = np.array([[0, 0, 1], [1, 0, 0]], f32)
    Nn = np.array([[0, 0, -1], [-1, 0, 0]], f32)
    out, st = OM.orient(P, Nn, 2)
    assert st["levels"] == [0, 0, 0, 1] and out[0, 2] == 1 and out[1, 0] == -1
    # the seed's n_z == 0 rule
    out, st = OM.orient(P[:1], np.array([[0.5, -0.75, 0]], f32), 2)
    assert list(out[0]) == [-0.5, 0.75, 0] and st["rounds"] == 5 and st["flipped"] == 1


# ---- the kernels' decisions, built for the host ----
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("points_orient_host")
    exe = str(d / "points_orient_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "points_orient_host.cpp"), "-o", exe])

    def run(mode, data):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        data.tofile(fin)
        p = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and f"points_orient_host {mode} ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
        return np.fromfile(fout, np.int32)
    return run


def _unit(rs, shape):
    v = rs.standard_normal(shape + (3,))
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def choose_cases():
    """-> found, round, level, n_i (cases, 3), rows (cases, 64, 5: n_j, stamp, sign): random rows; ties in |dot|; dot == 0; a weight
    exactly at each threshold; invalid normals (zero, NaN, inf) with and without stamps."""
    rs = np.random.default_rng(21)
    cases = 4000
    kind = rs.integers(0, 5, cases)
    found = rs.choice([0, 1, 2, 4, 8, 9, 16, 33, 64], cases).astype(np.int64)
    rnd = rs.integers(2, 40, cases)
    level = rs.integers(0, 4, cases)
    ni = _unit(rs, (cases,))
    nj = _unit(rs, (cases, 64))
    near = rs.random((cases, 64)) < 0.5                   # many neighbours nearly parallel, so that every level accepts some
    nj = np.where(near[..., None], (ni[:, None, :] * rs.choice([-1, 1], (cases, 64, 1)) + 0.2 * nj).astype(f32), nj)
    stamp = rs.integers(0, 45, (cases, 64))              # 0: unoriented; some >= the round
    sign = rs.choice([-1, 1], (cases, 64))
    # 1: ties -- axis-aligned and dyadic normals, copies and negated copies within the row
    t = kind == 1
    ni[t] = rs.choice([-1, -0.5, 0, 0.5, 1], (int(t.sum()), 3)).astype(f32)
    nj[t] = rs.choice([-1, -0.5, 0, 0.5, 1], (int(t.sum()), 64, 3)).astype(f32)
    # 2: a dot of exactly 0 for every source
    z = kind == 2
    ni[z] = np.array([0, 0, 1], f32)
    nj[z, :, 2] = 0
    # 3: the best weight exactly at a threshold: n_i = e_z, n_j = (0, 0, +-T) or the value next to it, the others smaller
    e = kind == 3
    T = np.array(OM.LEVELS)
    ni[e] = np.array([0, 0, 1], f32)
    nj[e] = (nj[e] * f32(0.25)).astype(f32)
    pick = rs.integers(0, 4, int(e.sum()))
    w = T[pick].astype(f32)
    w = np.where(rs.random(len(w)) < 0.5, w, np.nextafter(w, rs.choice([f32(-1), f32(2)], len(w)).astype(f32)))
    first = np.zeros((int(e.sum()), 3), f32)
    first[:, 2] = w * rs.choice([-1, 1], len(w))
    nj[e, 0] = first
    stamp[e, 0] = 1
    level[e] = np.where(rs.random(int(e.sum())) < 0.7, pick, level[e])
    found[e] = np.maximum(found[e], 1)
    # 4: invalid normals scattered, stamped or not
    v = kind == 4
    bad = np.array([[0, 0, 0], [-0.0, 0, -0.0], [np.nan, 0, 1], [0, np.inf, 0], [1, 0, -np.inf]], f32)
    hit = v[:, None] & (rs.random((cases, 64)) < 0.4)
    nj[hit] = bad[rs.integers(0, len(bad), int(hit.sum()))]
    rows = np.concatenate([nj, stamp[..., None].astype(f32), sign[..., None].astype(f32)], axis=-1).astype(f32)
    return found, rnd, level, ni, rows


def test_host_choice_equals_the_model(host):
    found, rnd, level, ni, rows = choose_cases()
    cases = len(found)
    flat = np.concatenate([found[:, None].astype(f32), rnd[:, None].astype(f32), level[:, None].astype(f32), ni, rows.reshape(cases, -1)], axis=1)
    out = host("choose", np.concatenate([np.array([cases], f32), flat.astype(f32).reshape(-1)])).reshape(cases, 2)
    acc = np.zeros(cases, bool)
    sg = np.zeros(cases, np.int64)
    for L in range(4):                       # (the model takes one threshold per call)
        for r in np.unique(rnd):
            m = (level == L) & (rnd == r)
            a, s = OM.choose(ni[m], rows[m, :, :3], rows[m, :, 3].astype(np.int64), rows[m, :, 4].astype(np.int64), found[m], int(r), OM.LEVELS[L])
            acc[m], sg[m] = a, s
    assert np.array_equal(out[:, 0] != 0, acc) and np.array_equal(out[acc, 1], sg[acc])
    assert acc.any() and (~acc).any() and (sg[acc] < 0).any() and (sg[acc] > 0).any()


def test_host_seed_rules_equal_the_model(host):
    rs = np.random.default_rng(22)
    Nn = rs.standard_normal((600, 3)).astype(f32)
    Nn[:200] = rs.choice([-1, -0.5, 0, -0.0, 0.5, 1], (200, 3)).astype(f32)          # n_z == 0, ties of magnitude, all zero
    Nn[200:230, rs.integers(0, 3, 30)] = np.nan
    Nn[230:260, 1] = rs.choice([np.inf, -np.inf], 30)
    out = host("seed", np.concatenate([np.array([len(Nn)], f32), Nn.reshape(-1)])).reshape(-1, 3)
    ok = OM.valid(Nn)
    assert np.array_equal(out[:, 0] != 0, ok) and ok.any() and (~ok).any()
    assert np.array_equal(out[ok, 1], OM.seed_sign(Nn[ok]))
    assert ((Nn[ok][:, 2] == 0) & (np.abs(Nn[ok][:, 0]) == np.abs(Nn[ok][:, 1]))).any()   # a tie of magnitude under n_z == 0
    assert np.array_equal(out[:, 2].view(np.uint32), Nn[:, 0].copy().view(np.uint32) ^ np.uint32(0x80000000))
    # the order of seeds: greatest z, ties to the lowest index, -0 == +0, a NaN as -inf
    lists, length = 300, 40
    z = rs.choice([-2, -1, -0.0, 0, 1, 1.5, np.nan, -np.inf, np.inf, 3e38, -3e38, 1e-45, -1e-45], (lists, length)).astype(f32)
    cand = rs.random((lists, length)) < 0.6
    cand[:5] = False
    z[5:10] = np.nan
    out = host("pick", np.concatenate([np.array([lists, length], f32), np.stack([z, cand.astype(f32)], axis=-1).reshape(-1)]))
    assert list(out) == [OM.next_seed(z[i], cand[i]) for i in range(lists)]
    pairs = np.array([(l, c) for l in range(6) for c in (0, 1, 7)], np.int32)
    assert list(host("level", pairs.reshape(-1))) == [OM.next_level(int(l), int(c)) for l, c in pairs]


# ---- the C ABI ----
def test_orient_entry_points_exported():
    L = N.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in N.SIGNATURES, name


def test_orient_refuses_without_device():
    """No device (or sdfk_init not called): both entry points return SDFK_ERR_NO_DEVICE, in a fresh process."""
    p = subprocess.run([sys.executable, "-c", "from tests.test_orient_model import _refusals; _refusals(); print('refusals ok')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "refusals ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def _refusals():
    L = N.lib()
    a = np.zeros((3, 3), f32)
    A = C.c_void_p(a.ctypes.data)
    for name in ENTRY_POINTS:
        assert getattr(L, name)(None, 8, np.inf, 64, A, None) == N.ERR_NO_DEVICE, name
