"""CPU checks of the point-to-plane part of sdfkit_amd/csrc/icp_solve.h, built for the host with g++ -ffp-contract=off
(tests/cpp/icp_plane_host.cpp), against tests/icp_plane_model.py:

1. host build == model bit for bit: plane_row; lambda, x, the retained count, R, T, step, total and converged of the solve -- on
   random SPD matrices (normal equations of random correspondences, and Q diag Q^T with condition numbers up to 1e10), exactly
   rank-deficient ones (rank 3 from a plane with normals (0, 0, 1): rows and columns 2, 3, 4 are exactly zero; rank 5 from a
   cylinder along z with a non-circular profile: every n2 = 0, so row and column 5 are exactly zero), numerically rank-deficient
   ones (a tilted plane, a circular cylinder), A = 0, A and b scaled by 2^+-200, a diagonal A with an eigenvalue exactly ON the
   cut, and matrices whose null-space eigenvalues still move in the last sweep;
2. against LAPACK (np.linalg.eigh, another algorithm): x equals the truncated pseudo-inverse solution within 256 eps kappa |x|,
   kappa = lambda_max / the least retained eigenvalue -- 8 sweeps x 15 rotations x 2 roundings of a backward-stable iteration -- on
   the cases with no eigenvalue within a factor 10 of the cut;
3. R^T R = I within 24 eps.  With u = eps / 2 per rounding: ww carries 3u (relative, all terms positive), so 1 - ww has an absolute
   error of 3u ww + u |1 - ww| and 1 + ww a relative one of 4u; a diagonal numerator (1 - ww) + 2 w_a w_a adds u 2 w_a w_a + u |num|,
   an off-diagonal one 2 w_a w_b -+ 2 w_c has u 2 |w_a w_b| + u |num|; the division adds u.  Divided by 1 + ww >= max(ww, |1 - ww|,
   2 |w_a w_b|) and with |R_ab| <= 1: |dR_aa| <= (3 + 1 + 2 + 1 + 5) u = 12 u, |dR_ab| <= 7 u.  (R^T R - I)_ab = sum_k R_ka dR_kb +
   dR_ka R_kb, and a column of R has 1-norm <= sqrt(3): <= 2 sqrt(3) 12 u = 41.6 u = 20.8 eps, 24 eps with the second-order terms.
   It holds for every w (the formula has no small-angle assumption): |x[0..2]| from 0 to 1e12 is in the cases;
4. the plane case in the model: x[2] == x[3] == x[4] == 0 exactly and 3 eigenvalues retained;
5. tests/golden/icp_plane_cases.json is what the two models give for the height-field case at n = 700;
6. single textual mutations of the header are each detected:

   mutation            the one-line change                                  noticed by
   cross_swapped       c = n x d instead of d x n                           row == model
   no_centring         d = p instead of p - pmean                           row == model
   plus_b              nb = +b                                              solve == model, LAPACK
   w_is_x              w = x instead of x / 2                               solve == model (R, T, step, total)
   one_sweep_fewer     kSweeps6 - 1 sweeps                                  solve == model: the eigenvalues of the SLOW cases, whose
                                                                            null-space entries still move in sweep 8 (asserted in the
                                                                            model); x itself stops changing a sweep earlier, which is
                                                                            the margin kSweeps6 leaves
   cut_ge              lambda_k >= cut for lambda_k > cut                   solve == model on the on-cut case: diag(1, 1e-12, ...),
                                                                            where fl(1e-12 * 1) == 1e-12 sits exactly on the cut
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import icp_plane_model as M
from tests import points_model as PM
from tests.test_icp_solve import same_bits, write_cases

f32, f64 = np.float32, np.float64
EPS = np.finfo(f64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "sdfkit_amd", "csrc", "icp_solve.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "icp_plane_cases.json")
ROW_IN, ROW_OUT, SOLVE_IN, SOLVE_OUT = 12, 7, 48, 58


def build_host(d, header_text=None, tag="shipped"):
    """g++ build of tests/cpp/icp_plane_host.cpp; with `header_text`, against that text in place of icp_solve.h."""
    d = str(d)
    src = os.path.join(ROOT, "tests", "cpp", "icp_plane_host.cpp")
    if header_text is not None:
        tree = os.path.join(d, tag)
        os.makedirs(os.path.join(tree, "tests", "cpp"))
        os.makedirs(os.path.join(tree, "sdfkit_amd", "csrc"))
        shutil.copy(src, os.path.join(tree, "tests", "cpp"))
        shutil.copy(os.path.join(ROOT, "sdfkit_amd", "csrc", "points_knn.h"), os.path.join(tree, "sdfkit_amd", "csrc"))
        with open(os.path.join(tree, "sdfkit_amd", "csrc", "icp_solve.h"), "w") as f:
            f.write(header_text)
        src = os.path.join(tree, "tests", "cpp", "icp_plane_host.cpp")
    exe = os.path.join(d, "icp_plane_host_" + tag)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", src, "-o", exe])
    return exe


def runner(exe, d):
    def run(mode, rows):
        nout = {"row": ROW_OUT, "solve": SOLVE_OUT}[mode]
        fin, fout = os.path.join(str(d), f"{mode}.in"), os.path.join(str(d), f"{mode}.out")
        write_cases(fin, rows, f64)
        p = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and f"icp_plane_host {mode} ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        return np.fromfile(fout, f64).reshape(len(rows), nout)
    return run


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("icp_plane_host")
    return runner(build_host(d), d)


# ---- the cases ----
def pack21(A):
    return np.array([A[a, b] for a, b in M.UPPER6], f64)


def _normal_equations(p, q, n):
    """A, b, pmean of correspondences (float32 values), accumulated with the model's row in plain order"""
    p, q, n = [np.asarray(v, f32) for v in (p, q, n)]
    pmean = p.astype(f64).sum(axis=0) / len(p)
    A, b = np.zeros((6, 6)), np.zeros(6)
    for i in range(len(p)):
        J, r = M.plane_row_exact(p[i], q[i], n[i], pmean)
        A += np.outer(J, J)
        b += J * r
    return A, b, pmean


def _orthogonal(rs):
    return np.linalg.qr(rs.standard_normal((6, 6)))[0]


SLOW_SEEDS = [1041, 1756, 3522, 3727, 5926, 6341, 8372, 8877]


def slow_matrix(seed):
    """rank-deficient Q diag Q^T found by a search over 12 000 seeds: lambda or V still change in sweep 9 of a longer run"""
    rs = np.random.default_rng(seed)
    Q = _orthogonal(rs)
    rank = 1 + seed % 5
    s = np.zeros(6)
    s[:rank] = rs.uniform(0.5, 2, rank)
    A = (Q * s) @ Q.T
    return (A + A.T) / 2


def solve_cases():
    """-> (rows (cases, SOLVE_IN), kind per row)"""
    rs = np.random.default_rng(7)
    As, bs, pms, kind = [], [], [], []

    def add(A, b, pm, k):
        As.append(np.asarray(A, f64)); bs.append(np.asarray(b, f64)); pms.append(np.asarray(pm, f64)); kind.append(k)

    for _ in range(60):                                        # normal equations of random correspondences
        n = int(rs.integers(8, 60))
        p = rs.uniform(-1, 1, (n, 3))
        nn = rs.standard_normal((n, 3))
        nn /= np.linalg.norm(nn, axis=1, keepdims=True)
        add(*_normal_equations(p, p + rs.normal(0, 0.01, (n, 3)), nn), "spd")
    for _ in range(80):                                        # Q diag Q^T, condition up to 1e10
        Q = _orthogonal(rs)
        s = 10.0 ** rs.uniform(-10, 0, 6)
        A = (Q * s) @ Q.T
        add((A + A.T) / 2, rs.standard_normal(6), rs.standard_normal(3), "graded")
    for _ in range(20):                                        # large steps: |x| up to 1e3
        Q = _orthogonal(rs)
        s = rs.uniform(0.5, 2.0, 6)
        A = (Q * s) @ Q.T
        add((A + A.T) / 2, rs.standard_normal(6) * 10.0 ** rs.uniform(0, 3), rs.standard_normal(3), "large")
    for _ in range(10):                                        # a plane with normals (0, 0, 1): exactly rank 3
        n = 40
        p = np.concatenate([rs.uniform(-1, 1, (n, 2)), rs.normal(0.1, 0.01, (n, 1))], axis=1)
        q = p * np.array([1, 1, 0])
        add(*_normal_equations(p, q, np.tile([0.0, 0.0, 1.0], (n, 1))), "plane_exact")
    for _ in range(10):                                        # a tilted plane: rank 3 up to rounding
        n = 40
        nrm = rs.standard_normal(3)
        nrm /= np.linalg.norm(nrm)
        u = np.linalg.svd(nrm[None])[2][1:]
        p = rs.uniform(-1, 1, (n, 2)) @ u + nrm * rs.normal(0.1, 0.01, (n, 1))
        add(*_normal_equations(p, p - nrm * 0.1, np.tile(nrm, (n, 1))), "plane_tilted")
    for _ in range(10):                                        # an elliptic cylinder along z: n2 = 0 exactly, rank 5 exactly
        n = 60
        phi, z = rs.uniform(0, 2 * np.pi, n), rs.uniform(-1, 1, n)
        p = np.stack([2 * np.cos(phi), np.sin(phi), z], axis=1)
        nn = np.stack([np.cos(phi) / 2, np.sin(phi), np.zeros(n)], axis=1)
        nn /= np.linalg.norm(nn, axis=1, keepdims=True)
        add(*_normal_equations(p + rs.normal(0, 0.01, (n, 3)), p, nn), "cylinder_exact")
    for _ in range(10):                                        # a circular cylinder: the rotation about z is unobserved as well
        n = 60
        phi, z = rs.uniform(0, 2 * np.pi, n), rs.uniform(-1, 1, n)
        nn = np.stack([np.cos(phi), np.sin(phi), np.zeros(n)], axis=1)
        p = nn + np.array([0, 0, 1]) * z[:, None]
        add(*_normal_equations(p + nn * rs.normal(0, 0.01, (n, 1)), p, nn), "cylinder_round")   # (radial offsets: p x n stays along z-free)
    add(np.zeros((6, 6)), rs.standard_normal(6), rs.standard_normal(3), "zero")
    add(np.zeros((6, 6)), np.zeros(6), np.zeros(3), "zero")
    for k in range(6):                                         # A and b scaled by 2^+-200
        for e in (200, -200):
            add(np.ldexp(As[k], e), np.ldexp(bs[k], e), pms[k], "scaled")
    add(np.diag([1.0, 1e-12, 0.5, 0.25, 0.125, 1.0]), np.ones(6), np.zeros(3), "on_cut")
    add(np.diag([1.0, np.nextafter(1e-12, 1.0), 0.5, 0.25, 0.125, 1.0]), np.ones(6), np.zeros(3), "above_cut")
    for seed in SLOW_SEEDS:
        add(slow_matrix(seed), np.random.default_rng(seed).standard_normal(6), np.zeros(3), "slow")
    n = len(As)
    rows = np.zeros((n, SOLVE_IN))
    rows[:, :21] = [pack21(A) for A in As]
    rows[:, 21:27] = bs
    rows[:, 27:30] = pms
    prev = np.tile(np.eye(4, dtype=f32), (n, 1, 1))
    for c in range(n):
        prev[c, :3, :3] = np.linalg.qr(rs.standard_normal((3, 3)))[0].astype(f32)
        prev[c, 3, :3] = rs.standard_normal(3).astype(f32)
    rows[:, 30:46] = prev.reshape(n, 16)
    rows[:, 46], rows[:, 47] = f32(1e-4), f32(1e-5)
    rows[::7, 46], rows[::7, 47] = f32(1e30), f32(1e30)
    return rows, kind


def model_solve(rows, sweeps=M.SWEEPS6):
    out = np.zeros((len(rows), SOLVE_OUT))
    for c, r in enumerate(rows):
        x, retained, lam, R, T, step, total, conv = M.solve_step_plane_exact(r[:21], r[21:27], r[27:30], r[30:46].astype(f32), f32(r[46]), f32(r[47]),
                                                                             sweeps=sweeps)
        out[c, :6], out[c, 6:12], out[c, 12], out[c, 13:22], out[c, 22:25] = lam, x, retained, R.reshape(-1), T
        out[c, 25:41], out[c, 41:57], out[c, 57] = step.reshape(-1), total.reshape(-1), conv
    return out


def row_cases():
    rs = np.random.default_rng(17)
    rows = np.zeros((400, ROW_IN))
    rows[:, :9] = rs.uniform(-2, 2, (400, 9)).astype(f32)
    rows[:, 9:] = rs.uniform(-1, 1, (400, 3))
    rows[:20, 6:9] = 0.0                                       # zero normals: J = 0, r = 0
    rows[20:40, 9:] = 0.0
    return rows


def model_rows(rows):
    out = np.zeros((len(rows), ROW_OUT))
    for c, r in enumerate(rows):
        out[c, :6], out[c, 6] = M.plane_row_exact(r[:3], r[3:6], r[6:9], r[9:12])
    return out


@pytest.fixture(scope="module")
def solved(host):
    rows, kind = solve_cases()
    return rows, kind, host("solve", rows), model_solve(rows)


# ---- 1. bit-equality with the model ----
def test_host_rows_equal_the_model(host):
    rows = row_cases()
    got, want = host("row", rows), model_rows(rows)
    assert same_bits(got, want).all()
    assert (np.abs(want[40:, :6]).min(axis=0) > 0).all()


def test_host_solve_equals_the_model(solved):
    rows, kind, got, want = solved
    bad = np.flatnonzero(~same_bits(got, want).all(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], [kind[c] for c in bad[:5]], got[bad[0]], want[bad[0]])


def test_cases_reach_every_branch(solved):
    rows, kind, got, want = solved
    kind = np.array(kind)
    ret = want[:, 12]
    assert (ret[kind == "spd"] == 6).all() and (ret[kind == "large"] == 6).all()
    assert (ret[kind == "plane_exact"] == 3).all() and (ret[kind == "plane_tilted"] == 3).all()
    assert (ret[kind == "cylinder_exact"] == 5).all() and (ret[kind == "cylinder_round"] == 4).all()
    for c in np.flatnonzero(kind == "plane_exact"):
        A = M.unpack21(rows[c, :21])
        assert (A[2:5] == 0).all() and (A[:, 2:5] == 0).all() and (want[c, 6 + 2:6 + 5] == 0).all()
    for c in np.flatnonzero(kind == "cylinder_exact"):
        A = M.unpack21(rows[c, :21])
        assert (A[5] == 0).all() and (A[:, 5] == 0).all() and want[c, 6 + 5] == 0
    z = np.flatnonzero(kind == "zero")
    assert (ret[z] == 0).all() and (want[z, 6:12] == 0).all() and np.array_equal(want[z[0], 13:22].reshape(3, 3), np.eye(3))
    assert want[z[1], 57] == 1.0 and np.array_equal(want[z[1], 25:41].reshape(4, 4), np.eye(4))   # x = 0 at pmean = 0: the identity, converged
    # 2^+-200: the same x (every operation of the Jacobi and of the solve scales exactly while nothing leaves the normal range)
    s = np.flatnonzero(kind == "scaled")
    assert (ret[s] == 6).all() and np.allclose(want[s, 6:12], np.repeat(want[:6, 6:12], 2, axis=0), rtol=1e-9, atol=0)
    on, above = np.flatnonzero(kind == "on_cut")[0], np.flatnonzero(kind == "above_cut")[0]
    assert M.TAU * f64(1.0) == f64(1e-12) and ret[on] == 5 and want[on, 6 + 1] == 0 and ret[above] == 6 and want[above, 6 + 1] != 0
    # the slow cases: one sweep fewer gives other eigenvalues, but the same x
    slow = np.flatnonzero(kind == "slow")
    fewer = model_solve(rows[slow], M.SWEEPS6 - 1)
    assert not same_bits(fewer[:, :6], want[slow, :6]).all() and same_bits(fewer[:, 6:12], want[slow, 6:12]).all()
    assert 0 < want[:, 57].sum() < len(want)


# ---- 2. against LAPACK ----
def lapack_failures(rows, got):
    bad = []
    for c, r in enumerate(rows):
        A, b = M.unpack21(r[:21]), r[21:27]
        w, V = np.linalg.eigh(A)
        if not (w.max() > 0 and np.isfinite(w.max())):
            continue
        cut = 1e-12 * w.max()
        if ((np.abs(w) > cut / 10) & (np.abs(w) < cut * 10)).any():
            continue                                           # (an eigenvalue at the cut: which side it falls on is the algorithm's)
        keep = w > cut
        x = (V[:, keep] * (V[:, keep].T @ -b / w[keep])).sum(axis=1)
        kappa = w.max() / w[keep].min()
        err = np.abs(got[c, 6:12] - x).max()
        if not err <= 256 * EPS * kappa * np.abs(x).max() or got[c, 12] != keep.sum():
            bad.append((c, err / (EPS * kappa * max(np.abs(x).max(), 1e-300)), got[c, 12], keep.sum()))
    return bad


def test_solve_against_lapack(solved):
    rows, kind, got, want = solved
    assert not lapack_failures(rows, got)


# ---- 3. orthogonality ----
def test_cayley_rotation_is_orthogonal(solved):
    rows, kind, got, want = solved
    worst = 0.0
    for c in range(len(rows)):
        R = got[c, 13:22].reshape(3, 3)
        worst = max(worst, np.abs(R.T @ R - np.eye(3)).max())
        assert abs(np.linalg.det(R) - 1.0) <= 24 * EPS
    big = np.abs(got[:, 6:9]).max(axis=1)
    print("R^T R - I: worst", worst / EPS, "eps; largest |x[0..2]|", big.max())
    assert worst <= 24 * EPS and big.max() > 100


# ---- 4. the plane case ----
def test_plane_case_in_the_model():
    S, Nn, D = M.plane_case()
    assert np.array_equal(PM.nearest(S, D)[0], np.arange(len(S)))
    total, iters, totals, infos = M.register_plane_exact(S, Nn, D.copy())
    assert 1 <= iters < 10
    for info in infos:
        A, x = info["A"], info["x"]
        assert (A[2:5] == 0).all() and (A[:, 2:5] == 0).all() and info["retained"] == 3 and info["kept"] == len(S)
        assert x[2] == 0 and x[3] == 0 and x[4] == 0
    assert np.abs(infos[-1]["points"][:, 2]).max() <= 1e-6     # on the plane; x and y are free and stay where they were
    assert x[0] != 0 or infos[0]["x"][0] != 0


# ---- 5. the recorded worth ----
def golden_cases():
    S, Nn = M.height_field_static()
    D0, D = M.height_field_dynamic(700)
    pts = D.copy()
    _, it_point, _, _ = PM.register_exact(S, pts)
    rms_point = M.rms(pts, D0)
    pts = D.copy()
    _, it_plane, _, _ = M.register_plane_exact(S, Nn, pts)
    return {"case": "height field 48 x 48, n = 700, default limits",
            "point": {"iterations": it_point, "rms": rms_point}, "plane": {"iterations": it_plane, "rms": M.rms(pts, D0)}}


def test_golden_cases_are_the_models():
    with open(GOLDEN) as f:
        rec = json.load(f)
    now = golden_cases()
    for metric in ("point", "plane"):
        assert now[metric]["iterations"] == rec[metric]["iterations"]
        assert abs(now[metric]["rms"] - rec[metric]["rms"]) <= 1e-6 * rec[metric]["rms"]
    assert rec["plane"]["iterations"] < rec["point"]["iterations"] and rec["plane"]["rms"] < rec["point"]["rms"]


# ---- 6. mutations of the header ----
def _sub(old, new):
    def f(t):
        assert t.count(old) == 1, (old, t.count(old))
        return t.replace(old, new)
    return f


MUTATIONS = [
    ("cross_swapped", _sub("J[0] = d1 * n2 - d2 * n1; J[1] = d2 * n0 - d0 * n2; J[2] = d0 * n1 - d1 * n0;",
                           "J[0] = n1 * d2 - n2 * d1; J[1] = n2 * d0 - n0 * d2; J[2] = n0 * d1 - n1 * d0;"), {"row"}),
    ("no_centring", _sub("const double d0 = p0 - pmean[0], d1 = p1 - pmean[1], d2 = p2 - pmean[2];", "const double d0 = p0, d1 = p1, d2 = p2;"), {"row"}),
    ("plus_b", _sub("nb[a] = -b[a];", "nb[a] = b[a];"), {"model", "lapack"}),
    ("w_is_x", _sub("const double w0 = x[0] / 2.0, w1 = x[1] / 2.0, w2 = x[2] / 2.0;", "const double w0 = x[0], w1 = x[1], w2 = x[2];"), {"model"}),
    ("one_sweep_fewer", _sub("sweep < kSweeps6;", "sweep < kSweeps6 - 1;"), {"model"}),
    ("cut_ge", _sub("if (!(lam[k] > cut)) continue;", "if (!(lam[k] >= cut)) continue;"), {"model"}),
]


def test_mutations_of_the_header_are_detected(tmp_path):
    with open(HEADER) as f:
        text = f.read()
    rows, kind = solve_cases()
    want = model_solve(rows)
    rrows = row_cases()
    rwant = model_rows(rrows)
    for name, mutate, expected in MUTATIONS:
        run = runner(build_host(tmp_path, mutate(text), name), tmp_path)
        got = run("solve", rows)
        noticed = set()
        if not same_bits(run("row", rrows), rwant).all():
            noticed.add("row")
        if not same_bits(got, want).all():
            noticed.add("model")
        if lapack_failures(rows, got):
            noticed.add("lapack")
        print(f"{name:16s} noticed by: {sorted(noticed)}")
        assert expected <= noticed, (name, "NOT detected", noticed)
        if name == "cut_ge":                                   # the on-cut case alone tells the two comparisons apart
            differ = np.flatnonzero(~same_bits(got, want).all(axis=1))
            assert [kind[c] for c in differ] == ["on_cut"]
