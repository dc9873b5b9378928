"""CPU checks of the IterativeClosestPoint solve (sdfkit_amd/csrc/icp_solve.h), built for the host with g++:

1. the Kabsch solve against LAPACK (np.linalg.svd, another algorithm) on conditioning-independent quantities: orthogonality,
   det R = +1, Kabsch's optimum tr(R C) = s0 + s1 + sign(det C) s2, and for rank 1 the direction of the p line going to that of
   the q line -- over eight classes of C = A diag(s) B^T and hand-made exact cases;
2. kabsch_r(C 2^k) == kabsch_r(C) bit for bit for every k that keeps |C| within [2^-300, 2^289];
3. the host build == the numpy transcription (tests/points_model.py) bit for bit: R, step, total, converged; m4_invert / m4_mul ==
   Matrix4x4.Invert / Multiply; the distMax rule and the filter at every bracket boundary;
4. the fixed reduction order of the model (reduce_fixed) on hand-made sums;
5. single textual mutations of the header are each detected by 1 - 3.

The bounds of 1 are 64 eps: a few dozen roundings of quantities of size 1 (the numpy transcription's worst values over these
classes are 9 eps for R^T R - I and 16 eps for the optimum)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from sdfkit_amd.raymarch import Matrix4x4
from tests import points_model as PM

f32, f64 = np.float32, np.float64
EPS = np.finfo(f64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "sdfkit_amd", "csrc", "icp_solve.h")
SOLVE_IN, SOLVE_OUT, M4_IN, M4_OUT, FILTER_IN, FILTER_OUT = 33, 42, 32, 33, 7, 3


def same_bits(a, b):
    """bit-equal, or NaN on both sides (IEEE 754 leaves the payload and sign of a produced NaN open)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    u = np.uint64 if a.dtype == f64 else np.uint32
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


# ---- building and running the host program ----
def build_host(d, header_text=None, tag="shipped"):
    """g++ build of tests/cpp/icp_solve_host.cpp; with `header_text`, against that text in place of icp_solve.h."""
    d = str(d)
    src = os.path.join(ROOT, "tests", "cpp", "icp_solve_host.cpp")
    if header_text is not None:
        tree = os.path.join(d, tag)
        os.makedirs(os.path.join(tree, "tests", "cpp"))
        os.makedirs(os.path.join(tree, "sdfkit_amd", "csrc"))
        shutil.copy(src, os.path.join(tree, "tests", "cpp"))
        shutil.copy(os.path.join(ROOT, "sdfkit_amd", "csrc", "points_knn.h"), os.path.join(tree, "sdfkit_amd", "csrc"))
        with open(os.path.join(tree, "sdfkit_amd", "csrc", "icp_solve.h"), "w") as f:
            f.write(header_text)
        src = os.path.join(tree, "tests", "cpp", "icp_solve_host.cpp")
    exe = os.path.join(d, "icp_solve_host_" + tag)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", src, "-o", exe])
    return exe


def write_cases(path, rows, dtype):
    rows = np.ascontiguousarray(rows, dtype)
    np.concatenate([np.array([len(rows)], dtype), rows.reshape(-1)]).tofile(path)


def runner(exe, d, prefix=()):
    def run(mode, rows):
        dtype, nout = {"solve": (f64, SOLVE_OUT), "m4": (f32, M4_OUT), "filter": (f64, FILTER_OUT)}[mode]
        fin, fout = os.path.join(str(d), f"{mode}.in"), os.path.join(str(d), f"{mode}.out")
        write_cases(fin, rows, dtype)
        p = subprocess.run(list(prefix) + [exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and f"icp_solve_host {mode} ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        return np.fromfile(fout, dtype).reshape(len(rows), nout)
    return run


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("icp_solve_host")
    return runner(build_host(d), d)


# ---- the cases ----
CLASSES = ["generic", "graded", "near_equal", "rank2", "reflection", "rank1", "nearly_rank2", "scaled"]
PER_CLASS = 500


def _rotation(rs):
    q, r = np.linalg.qr(rs.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def class_matrices():
    """-> (C (n, 3, 3), class index per matrix): C = A diag(s) B^T, A and B random rotations"""
    rs = np.random.default_rng(2024)
    Cs, kind = [], []
    for ci, name in enumerate(CLASSES):
        for _ in range(PER_CLASS):
            A, B = _rotation(rs), _rotation(rs)
            s = np.sort(rs.uniform(0.1, 10.0, 3))[::-1]
            scale = 1.0
            if name == "graded":
                s = np.array([1.0, 1e-3, 1e-6]) * rs.uniform(0.5, 2.0)
            elif name == "near_equal":
                s = 1.0 + rs.uniform(-1e-9, 1e-9, 3)
            elif name == "rank2":
                s[2] = 0.0
            elif name == "reflection":
                A[:, 2] = -A[:, 2]                     # det C < 0
            elif name == "rank1":
                s[1] = s[2] = 0.0
            elif name == "nearly_rank2":
                s[2] = s[0] * 10.0 ** rs.uniform(-11, -8)
            elif name == "scaled":
                scale = 10.0 ** rs.uniform(-30, 30)
            Cs.append((A * s) @ B.T * scale)
            kind.append(ci)
    return np.array(Cs), np.array(kind)


def exact_matrices():
    """hand-made C: 0, I, -I, a reflection, rank 1 on an axis, columns in ascending order of norm (the sort permutes; with and
    without a reflection, and rank 1 with the column last), columns of equal norm (zeta == 0)"""
    z = np.zeros((3, 3))
    asc = np.array([[1.0, 0.5, 0.25], [0.0, 2.0, 1.0], [0.0, 0.0, 4.0]])
    return {
        "zero": z, "identity": np.eye(3), "minus_identity": -np.eye(3), "mirror_z": np.diag([1.0, 1.0, -1.0]),
        "rank1_x": np.diag([2.0, 0.0, 0.0]), "ascending": asc, "ascending_diag": np.diag([1.0, 2.0, 3.0]),
        "ascending_mirror": np.diag([1.0, 2.0, -3.0]), "rank1_last_column": np.outer([1.0, 2.0, 2.0], [0.0, 0.0, 3.0]),
        "equal_norms": np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.5], [2.0, 2.0, 1.0]]),
        "equal_norms_2": np.array([[3.0, 0.0, 4.0], [1.0, 5.0, 0.0], [4.0, 1.0, 3.0]]),
    }


def solve_rows(Cs, seed=5):
    """a row of the case file per C: random means, a random previous total, the default limits (every 7th: limits no step misses)"""
    rs = np.random.default_rng(seed)
    n = len(Cs)
    rows = np.zeros((n, SOLVE_IN))
    rows[:, :9] = np.asarray(Cs, f64).reshape(n, 9)
    rows[:, 9:15] = rs.standard_normal((n, 6))
    prev = np.tile(np.eye(4, dtype=f32), (n, 1, 1))
    for c in range(n):
        prev[c, :3, :3] = _rotation(rs).astype(f32)
        prev[c, 3, :3] = rs.standard_normal(3).astype(f32)
    rows[:, 15:31] = prev.reshape(n, 16)
    rows[:, 31], rows[:, 32] = f32(1e-4), f32(1e-5)
    rows[::7, 31], rows[::7, 32] = f32(1e30), f32(1e30)
    return rows


def all_solve_cases():
    """-> (rows, kind (class index, -1 for the hand-made ones), names of the hand-made ones)"""
    Cs, kind = class_matrices()
    ex = exact_matrices()
    Cs = np.concatenate([Cs, np.array(list(ex.values()))])
    kind = np.concatenate([kind, np.full(len(ex), -1)])
    rows = solve_rows(Cs)
    # identity C, equal means, identity total: the step is the identity and the registration has converged
    i = len(rows) - len(ex) + list(ex).index("identity")
    rows[i, 9:15] = 0.25
    rows[i, 15:31] = np.eye(4).reshape(-1)
    rows[i, 31], rows[i, 32] = f32(1e-4), f32(1e-5)
    return rows, kind, list(ex)


def model_solve(rows):
    out = np.zeros((len(rows), SOLVE_OUT))
    infos = []
    for c, r in enumerate(rows):
        info = {}
        R, step, total, conv = PM.solve_step_exact(r[:9], r[9:12], r[12:15], r[15:31].astype(f32), f32(r[31]), f32(r[32]), info)
        out[c, :9], out[c, 9:25], out[c, 25:41], out[c, 41] = R.reshape(-1), step.reshape(-1), total.reshape(-1), conv
        infos.append(info)
    return out, infos


@pytest.fixture(scope="module")
def solved(host):
    rows, kind, names = all_solve_cases()
    want, infos = model_solve(rows)
    return rows, kind, names, host("solve", rows), want, infos


# ---- 1. against LAPACK ----
def reference_failures(rows, kind, got):
    """the conditioning-independent checks of every case -> the list of failures (empty: all hold)"""
    bad = []
    for c, (r, k) in enumerate(zip(rows, kind)):
        C, R = r[:9].reshape(3, 3), got[c, :9].reshape(3, 3)
        U, s, Vt = np.linalg.svd(C)
        orth = np.abs(R.T @ R - np.eye(3)).max()
        det = abs(np.linalg.det(R) - 1.0)
        sign = 0.0 if s[2] <= 8 * EPS * s[0] else np.sign(np.linalg.det(U) * np.linalg.det(Vt))   # rank-deficient: 0
        opt = (s[0] + s[1] + sign * s[2]) - np.trace(R @ C)
        if not orth <= 64 * EPS:
            bad.append((c, int(k), "R^T R - I", orth / EPS))
        if not det <= 64 * EPS:
            bad.append((c, int(k), "det R - 1", det / EPS))
        if not opt <= 64 * EPS * s[0]:
            bad.append((c, int(k), "tr(R C) below the optimum", opt / (EPS * max(s[0], 1e-300))))
        if s[0] > 0 and s[1] <= 1e-12 * s[0]:          # rank 1: R itself is not unique; the p line goes to the q line
            line = np.abs(R @ U[:, 0] - Vt[0]).max()
            if not line <= 64 * EPS:
                bad.append((c, int(k), "rank 1: R u != v", line / EPS))
    return bad


def test_solve_against_lapack(solved):
    rows, kind, names, got, want, infos = solved
    assert not reference_failures(rows, kind, got)
    assert np.isfinite(got[:, :9]).all()


def test_cases_reach_every_branch(solved):
    """asserted in the model (which the host build equals bit for bit): the rank-1 completion, C = 0, d3 = -1, a sort that
    permutes, rotations with zeta == 0, and at most 6 sweeps"""
    rows, kind, names, got, want, infos = solved
    by = {n: infos[len(infos) - len(names) + i] for i, n in enumerate(names)}
    assert all(i["rank1"] for i, k in zip(infos, kind) if k == CLASSES.index("rank1")) and by["rank1_x"]["rank1"] and by["rank1_last_column"]["rank1"]
    # d3 = sign det V (det U = +1 by construction: u3 = u1 x u2 absorbs the sign of a reflection), so d3 = -1 goes with the parity of
    # the rotations and of the sort, not with det C: it has to occur in every class, and det R = +1 whatever it is
    for ci in range(len(CLASSES)):
        d3 = [i["d3"] for i, k in zip(infos, kind) if k == ci]
        assert 50 < d3.count(-1.0) < PER_CLASS - 50 and d3.count(0.0) == 0, (CLASSES[ci], d3.count(-1.0))
    assert by["zero"]["s0_zero"] and by["zero"]["d3"] == 1.0
    at = lambda n: got[len(rows) - len(names) + names.index(n), :9].reshape(3, 3)
    assert np.array_equal(at("mirror_z"), np.eye(3)) and np.array_equal(at("minus_identity"), np.diag([-1.0, -1.0, 1.0]))
    assert np.array_equal(at("identity"), np.eye(3))
    for n in ("ascending", "ascending_diag", "ascending_mirror", "rank1_last_column"):
        assert by[n]["ord"] != (0, 1, 2), n
    assert by["equal_norms"]["zeta_zero"] >= 1 and by["equal_norms_2"]["zeta_zero"] >= 1
    assert sum(i["ord"] != (0, 1, 2) for i in infos) > 1000
    assert max(i["sweeps"] for i in infos) <= 6
    z = len(rows) - len(names) + names.index("zero")
    assert np.array_equal(got[z, :9].reshape(3, 3), np.eye(3))
    i = len(rows) - len(names) + names.index("identity")
    assert got[i, 41] == 1.0 and np.array_equal(got[i, 9:25].reshape(4, 4), np.eye(4))
    assert 0 < want[:, 41].sum() < len(want)


# ---- 2. power-of-two scaling ----
def scaling_rows():
    """every 25th class matrix and the hand-made ones, each scaled so that its largest magnitude has the exponents below: the ends
    of the contract range [2^-300, 2^289], both sides of 2^+-256 (where al * be leaves binary64 without the scaling), and between"""
    Cs, _ = class_matrices()
    base = np.concatenate([Cs[::25], np.array(list(exact_matrices().values()))])
    base = base[np.abs(base).reshape(len(base), -1).max(axis=1) > 0]
    exps = [-300, -257, -256, -255, -129, -128, -1, 0, 1, 127, 128, 254, 255, 256, 257, 288]
    m = np.abs(base).reshape(len(base), -1).max(axis=1)
    e0 = np.frexp(m)[1] - 1
    scaled = np.array([[np.ldexp(C, int(e - e0[c])) for e in exps] for c, C in enumerate(base)])
    return base, scaled


def scaling_failures(run):
    base, scaled = scaling_rows()
    ref = run("solve", solve_rows(base))[:, :9]
    got = run("solve", solve_rows(scaled.reshape(-1, 3, 3)))[:, :9].reshape(len(base), -1, 9)
    same = same_bits(got, np.broadcast_to(ref[:, None, :], got.shape).copy()).all(axis=2)
    return [(int(c), int(k)) for c, k in zip(*np.nonzero(~same))]


def test_power_of_two_scaling_is_bit_exact(host):
    assert not scaling_failures(host)


# ---- 3. bit-equality with the model ----
def test_host_solve_equals_the_model(solved):
    rows, kind, names, got, want, infos = solved
    bad = np.flatnonzero(~same_bits(got, want).all(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], kind[bad[:5]], got[bad[0]], want[bad[0]])


def m4_rows():
    rs = np.random.default_rng(77)
    mats = []
    for _ in range(300):                               # random affine matrices
        m = np.eye(4, dtype=f32)
        m[:3, :3] = (_rotation(rs) * rs.uniform(0.2, 3.0, 3)).astype(f32)
        m[3, :3] = rs.standard_normal(3).astype(f32) * f32(10)
        mats.append(m)
    for _ in range(100):                               # any 4 x 4
        mats.append(rs.standard_normal((4, 4)).astype(f32))
    for _ in range(50):                                # singular: a repeated row, a zero column
        m = rs.standard_normal((4, 4)).astype(f32)
        m[rs.integers(0, 4)] = m[rs.integers(0, 4)] * f32(2)
        mats.append(m)
        m = rs.standard_normal((4, 4)).astype(f32)
        m[:, rs.integers(0, 4)] = 0
        mats.append(m)
    mats.append(np.zeros((4, 4), f32))
    lim = f32(1.1920929e-07)                           # determinants just either side of the limit: exactly d here
    for d in (lim, np.nextafter(lim, f32(0)), np.nextafter(lim, f32(1)), -lim, -np.nextafter(lim, f32(0)), -np.nextafter(lim, f32(1))):
        for at in range(4):
            m = np.eye(4, dtype=f32)
            m[at, at] = d
            mats.append(m)
    for v in (np.nan, np.inf, -np.inf):                # NaN and infinities
        for at in ((0, 0), (1, 2), (3, 1), (3, 3)):
            m = rs.standard_normal((4, 4)).astype(f32)
            m[at] = v
            mats.append(m)
    a = np.array(mats, f32)
    b = a[rs.permutation(len(a))]
    return np.concatenate([a.reshape(len(a), 16), b.reshape(len(a), 16)], axis=1)


def model_m4(rows):
    out = np.zeros((len(rows), M4_OUT), f32)
    with np.errstate(all="ignore"):
        for c, r in enumerate(rows):
            ok, inv = Matrix4x4.Invert(r[:16].reshape(4, 4))
            out[c, :16], out[c, 16], out[c, 17:] = inv.reshape(-1), ok, Matrix4x4.Multiply(r[:16].reshape(4, 4), r[16:].reshape(4, 4)).reshape(-1)
    return out


def m4_failures(run):
    rows = m4_rows()
    got, want = run("m4", rows), model_m4(rows)
    # the limit: |det| < 1.1920929e-07 is refused with the all-NaN matrix and false
    lim = [c for c, r in enumerate(rows) if np.array_equal(r[:16].reshape(4, 4) != 0, np.eye(4, dtype=bool)) and (np.abs(np.diag(r[:16].reshape(4, 4))) < 1).any()]
    assert len(lim) == 24
    for c in lim:
        below = np.abs(np.diag(rows[c, :16].reshape(4, 4))).min() < f32(1.1920929e-07)
        assert want[c, 16] == (not below) and np.isnan(want[c, :16]).all() == below
    assert 0 < (want[:, 16] == 0).sum() < len(want) and np.isnan(want[:, 17:]).any()
    return list(np.flatnonzero(~same_bits(got, want).all(axis=1)))


def test_host_matrix4x4_equals_raymarch(host):
    assert not m4_failures(host)


GOOD = f32(0.01)


def filter_rows():
    """m at good, 3 good and 6 good (the f32 products the rule compares with) and one ulp below each, far inside each bracket, with
    sd = 0 and sd > 0; dist at distMax and one ulp either side.  The f64 part: mean and sqsum whose roundings to f32 land there."""
    rows = []
    down = lambda x: np.nextafter(f32(x), f32(-1))
    up = lambda x: np.nextafter(f32(x), f32(10))
    edges = [GOOD, f32(3.0) * GOOD, f32(6.0) * GOOD]
    ms = [f32(0), f32(0.001), f32(0.02), f32(0.04), f32(1.0)] + [e for e in edges] + [down(e) for e in edges] + [up(e) for e in edges]
    for m in ms:
        for sd in (f32(0), f32(0.0025), f32(0.3)):
            dmax = PM.dist_max_exact(f64(m), f64(sd) * f64(sd) * 7.0, 7, GOOD)[0]
            for dist in (dmax, down(dmax), up(dmax), f32(0), f32(np.inf), f32(np.nan)):
                rows.append([m, sd, GOOD, dist, f64(m), f64(sd) * f64(sd) * 7.0, 7.0])
    return np.array(rows, f64), edges


def filter_failures(run):
    rows, edges = filter_rows()
    got = run("filter", rows)
    bad = []
    with np.errstate(all="ignore"):
        for c, r in enumerate(rows):
            m, sd, dist = f32(r[0]), f32(r[1]), f32(r[3])
            # the reference's rule, written out: `<` at every boundary, so m == good is the second bracket
            want = m + f32(3) * sd if m < edges[0] else m + f32(2) * sd if m < edges[1] else m + sd if m < edges[2] else (m + f32(0.5)) + sd
            model = PM.dist_max_exact(r[4], r[5], r[6], GOOD)
            sd64 = f32(np.sqrt(r[5] / r[6]))
            want64 = PM.dist_max_exact(r[4], f64(sd64) * f64(sd64), 1, GOOD)[0]
            ok = same_bits(f32(got[c, 0]), f32(want)) and got[c, 1] == float(dist <= want) and same_bits(f32(got[c, 2]), f32(model[0])) and \
                same_bits(f32(model[0]), f32(want64))
            if not ok:
                bad.append((c, list(r), list(got[c])))
    # the boundaries themselves: at m == edge the next bracket's formula, one ulp below the previous one's (sd = 0.3 tells them apart)
    sel = [c for c, r in enumerate(rows) if f32(r[1]) == f32(0.3) and c % 6 == 0]         # (the rows whose dist is the model's distMax)
    seen = {(float(f32(rows[c, 0])), float(f32(got[c, 0]))) for c in sel}
    for k, e in enumerate(edges):
        lo = np.nextafter(e, f32(-1))
        for pair in ((float(e), float([e + f32(2) * f32(0.3), e + f32(0.3), (e + f32(0.5)) + f32(0.3)][k])),
                     (float(lo), float([lo + f32(3) * f32(0.3), lo + f32(2) * f32(0.3), lo + f32(0.3)][k]))):
            if pair not in seen:
                bad.append(("boundary", k, pair))
    bad += [("dist == distMax is not kept", c) for c in sel if got[c, 1] != 1.0]
    return bad


def test_host_filter_at_every_boundary(host):
    assert not filter_failures(host)


# ---- 4. the reduction order ----
def test_reduce_fixed_order():
    """sums whose value depends on the order: element i goes to accumulator i % 65536, strides in order, then the trees"""
    big = 2.0 ** 60
    v = np.zeros(65536 * 2 + 3)
    v[0], v[65536], v[131072] = big, 1.0, -big          # one accumulator, in order: (big + 1) - big = 0
    assert PM.reduce_fixed(v) == 0.0
    v[:] = 0
    v[0], v[131072], v[65536] = big, 1.0, -big          # (big - big) + 1 = 1
    assert PM.reduce_fixed(v) == 1.0
    v[:] = 0
    v[0], v[128], v[1] = big, -big, 1.0                 # the tree's first level pairs thread t with t + 128: (big - big) + 1
    assert PM.reduce_fixed(v) == 1.0
    v[:] = 0
    v[0], v[1], v[128] = big, -big, 1.0                 # (big + 1) + (-big + 0) = 0: threads 0 and 1 meet at the last level
    assert PM.reduce_fixed(v) == 0.0
    v[:] = 0
    v[0], v[256], v[256 * 128] = big, 1.0, -big         # across blocks: block 0 pairs with block 128 first
    assert PM.reduce_fixed(v) == 1.0
    rs = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 65535, 65536, 65537, 200001):
        x = rs.standard_normal((n, 3))
        got = PM.reduce_fixed(x)
        assert got.shape == (3,) and np.abs(got - x.sum(axis=0)).max() <= 64 * EPS * np.abs(x).sum(axis=0).max()
        assert PM.reduce_fixed(x[:, 0]) == got[0]
    assert np.signbit(PM.reduce_fixed(np.full(5, -0.0))) == False   # noqa: E712  (accumulators start at +0.0)


# ---- 5. mutations of the header ----
def _sub(old, new):
    def f(t):
        assert t.count(old) == 1, (old, t.count(old))
        return t.replace(old, new)
    return f


# name, mutation, the checks that must notice (any of them)
MUTATIONS = [
    ("filter_lt", _sub("return dist <= dmax;", "return dist < dmax;"), {"filter"}),
    ("d3_plus_one", _sub("const double d3 = detv > 0 ? 1.0 : (detv < 0 ? -1.0 : 0.0);", "const double d3 = 1.0;"), {"lapack", "model"}),
    ("no_sort", _sub("if (sg[ord[j]] < sg[ord[j + 1]]) { const int t = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = t; }", ";"), {"lapack", "model"}),
    ("completion_is_e", _sub("U[k][1] = w[k] / l;", "U[k][1] = e[k];"), {"lapack", "model"}),
    ("one_sweep", _sub("sweep < 60", "sweep < 1"), {"lapack", "model"}),
    ("zeta_gt", _sub("(zeta >= 0 ? 1.0 : -1.0)", "(zeta > 0 ? 1.0 : -1.0)"), {"model"}),
    # the header before the fix: al * be overflows (or underflows to 0) for |C| beyond 2^+-256
    ("no_scaling", _sub("W[a][b] = (C[3 * a + b] * f1) * f2;", "W[a][b] = C[3 * a + b];"), {"scaling"}),
    ("det_limit_le", _sub("fabsf(det) < 1.1920929e-07f", "fabsf(det) <= 1.1920929e-07f"), {"m4"}),
    ("bracket_le", _sub("if (m < good) dmax", "if (m <= good) dmax"), {"filter"}),
]


def test_mutations_of_the_header_are_detected(tmp_path):
    with open(HEADER) as f:
        text = f.read()
    rows, kind, names = all_solve_cases()
    want, _ = model_solve(rows)
    for name, mutate, expected in MUTATIONS:
        run = runner(build_host(tmp_path, mutate(text), name), tmp_path)
        got = run("solve", rows)
        noticed = set()
        if reference_failures(rows, kind, got):
            noticed.add("lapack")
        if not same_bits(got, want).all():
            noticed.add("model")
        if scaling_failures(run):
            noticed.add("scaling")
        if m4_failures(run):
            noticed.add("m4")
        if filter_failures(run):
            noticed.add("filter")
        print(f"{name:16s} noticed by: {sorted(noticed)}")
        assert noticed & expected, (name, "NOT detected", noticed)
        assert expected <= noticed or name == "no_scaling", (name, noticed)
