"""CPU check of the triangle-mesh distance arithmetic (sdfkit_amd/csrc/trimesh_sdf.h, the functions the kernels call, built with
g++ -ffp-contract=off by tests/cpp/trimesh_sdf_host.cpp) against the numpy model (tests/meshsdf_model.py), bit for bit: the
binary64 closest point on random, needle, collinear, coincident-vertex and zero-area triangles with queries at vertices, on edges
and on faces; exact orient2d signs on near-degenerate inputs; the perturbed column test and z_cross; col_range against every
coordinate of the axis."""
import os
import subprocess

import numpy as np
import pytest

from tests import meshsdf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trimesh") / "trimesh_sdf_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "trimesh_sdf_host.cpp"),
                           "-o", exe])
    return exe


def _run(exe, mode, rows, tmp_path, out_dtype, out_cols):
    src, dst = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
    np.ascontiguousarray(rows, f32).tofile(src)
    p = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "trimesh ok" in p.stdout, p.stderr
    return np.fromfile(dst, out_dtype).reshape(-1, out_cols)


def _triangles(rng):
    tris = [rng.uniform(-2, 2, (400, 3, 3))]
    base = rng.uniform(-1, 1, (60, 3))
    d = rng.uniform(-1, 1, (60, 3))
    tris.append(np.stack([base, base + d, base + d * 1e-6 + rng.uniform(-1e-7, 1e-7, (60, 3))], 1))   # needles
    tris.append(np.stack([base, base + d, base + 2 * d], 1))                                        # collinear
    tris.append(np.stack([base, base, base + d], 1))                                                # coincident vertices
    tris.append(np.stack([base, base, base], 1))                                                    # a point
    tris.append(np.stack([base, base + d, base + d * f32(0.5)], 1))                                  # zero area
    big = rng.uniform(-1, 1, (40, 3, 3)) * 1e6
    tris.append(big)
    return np.concatenate(tris).astype(f32)


def _queries(rng, T):
    n = len(T)
    w = rng.dirichlet([1, 1, 1], n)
    q = [rng.uniform(-3, 3, (n, 3)),
         T[np.arange(n), rng.integers(0, 3, n)],                                     # at a vertex
         (T[:, 0] * f32(0.5) + T[:, 1] * f32(0.5)),                                   # on an edge
         np.einsum("nk,nkc->nc", w, T),                                               # on the face
         np.einsum("nk,nkc->nc", w, T) + rng.normal(0, 1e-3, (n, 3))]                 # just off the face
    return [x.astype(f32) for x in q]


def test_closest_point_matches_model_bitwise(host_exe, tmp_path):
    rng = np.random.default_rng(7)
    T = _triangles(rng)
    rows = []
    for Q in _queries(rng, T):
        rows.append(np.concatenate([Q, T.reshape(-1, 9)], 1))
    rows = np.concatenate(rows)
    got = _run(host_exe, "closest", rows, tmp_path, np.float64, 7)
    p, a, b, c = [rows[:, 3 * k:3 * k + 3].astype(np.float64) for k in range(4)]
    d2, cp, w = M.closest_on_triangle(p, a, b, c)
    want = np.concatenate([d2[:, None], cp, w], 1)
    bad = np.nonzero(np.any(got.view(np.uint64) != want.view(np.uint64), axis=1))[0]
    assert len(bad) == 0, (len(bad), rows[bad[:3]], got[bad[:3]], want[bad[:3]])
    assert np.all(np.isfinite(got))
    # the degenerate ones are measured as edges: the distance is the least segment distance
    assert np.all(got[:, 0] >= 0)


def _orient_cases(rng):
    rows = [rng.uniform(-1, 1, (300, 6))]
    # nearly collinear: p on the segment ab up to one ulp, coordinates of very different magnitudes
    a = rng.uniform(-1, 1, (300, 2)) * np.array([1e-3, 1e3])
    b = rng.uniform(-1, 1, (300, 2)) * np.array([1e5, 1e-2])
    t = rng.uniform(0, 1, (300, 1))
    p = (a + t * (b - a)).astype(f32)
    rows.append(np.concatenate([a, b, p], 1))
    # exactly collinear on a grid, and points on the lines of axis-aligned edges
    g = rng.integers(-8, 8, (300, 6)).astype(float) * 0.25
    g[:, 4] = g[:, 0]
    rows.append(g)
    rows.append(np.array(_textbook_failure())[None])
    return np.concatenate(rows).astype(f32)


def _textbook_failure():
    """An input on which the textbook formula (bx-ax)*(py-ay) - (by-ay)*(px-ax) in f32 gets the sign wrong."""
    return [0.5000008940696716, 0.5000030398368835, 12.0, 12.0, 24.0000057220459, 24.000003814697266]


def test_orient2d_exact_matches_fractions(host_exe, tmp_path):
    rows = _orient_cases(np.random.default_rng(3))
    got = _run(host_exe, "orient", rows, tmp_path, np.int32, 2)
    ref = np.array([M.orient2d_fraction(*r) for r in rows])
    assert np.array_equal(got[:, 0], ref)
    assert np.array_equal(got[:, 0], M.orient2d_exact(*rows.T))
    assert np.array_equal(got[:, 1], M.orient2d_perturbed(*rows.T))
    assert np.all(got[:, 1] != 0) or np.all((got[:, 1] == 0) <= ((rows[:, 0] == rows[:, 2]) & (rows[:, 1] == rows[:, 3])))
    # the textbook f32 formula is wrong on the last case; the exact sign is not
    ax, ay, bx, by, px, py = [f32(x) for x in _textbook_failure()]
    naive = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    assert np.sign(naive) == -M.orient2d_fraction(*_textbook_failure()) != 0
    assert got[-1, 0] == M.orient2d_fraction(*_textbook_failure())


def test_column_inside_and_z_cross_match_model(host_exe, tmp_path):
    rng = np.random.default_rng(11)
    n = 2000
    T = rng.integers(-4, 5, (n, 3, 3)).astype(f32) * f32(0.5)        # vertices and columns on a shared lattice: ties
    T[: n // 2] = rng.uniform(-2, 2, (n // 2, 3, 3))
    P = rng.integers(-4, 5, (n, 2)).astype(f32) * f32(0.5)
    rows = np.concatenate([T.reshape(-1, 9), P], 1).astype(f32)
    got = _run(host_exe, "column", rows, tmp_path, np.float64, 2)
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    area = M.orient2d_exact(a[:, 0], a[:, 1], b[:, 0], b[:, 1], c[:, 0], c[:, 1])
    ins = (area != 0) & (M.orient2d_perturbed(a[:, 0], a[:, 1], b[:, 0], b[:, 1], P[:, 0], P[:, 1]) == area) & \
          (M.orient2d_perturbed(b[:, 0], b[:, 1], c[:, 0], c[:, 1], P[:, 0], P[:, 1]) == area) & \
          (M.orient2d_perturbed(c[:, 0], c[:, 1], a[:, 0], a[:, 1], P[:, 0], P[:, 1]) == area)
    assert np.array_equal(got[:, 0], area * 2 + ins)
    z = np.where(area != 0, M.z_cross(a, b, c, area, P[:, 0], P[:, 1]), 0.0)
    assert np.array_equal(got[:, 1].view(np.uint64), z.view(np.uint64))


def test_lattice_columns_counted_once_per_sheet():
    """Two triangles sharing an edge (a square split along its diagonal): every lattice column inside the square's projection,
    on its diagonal and edges included, is covered by exactly one of them under the perturbation rule."""
    V = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]], f32)
    T = np.array([0, 1, 2, 0, 2, 3], np.int32)
    d = np.array([0.5] * 3, f32)
    m = np.array([-1.0, -1.0, -1.0], f32)
    col, _ = M.crossings(V, T, m, d, 8, 8)
    xs = M.coord(m[0], np.arange(8), d[0])
    inside = [(i, j) for i in range(8) for j in range(8) if 0 <= xs[i] < 2 and 0 <= xs[j] < 2]
    assert sorted(col.tolist()) == sorted(i * 8 + j for i, j in inside)


def test_header_counts_each_lattice_column_once_per_sheet(host_exe, tmp_path):
    """The header's column test (the code the kernels run): for a square split along its diagonal, and for a fan of four
    triangles around a centre vertex, every lattice column -- on the shared edges and the shared vertex included -- lies in
    exactly one triangle of the sheet, or in none when it is outside the square."""
    sheets = {
        "diagonal": (np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]], f32), [(0, 1, 2), (0, 2, 3)]),
        "fan": (np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [1, 1, 0.5]], f32), [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)]),
    }
    ticks = np.arange(-2, 11, dtype=np.float32) * f32(0.25)
    cols = np.array([(x, y) for x in ticks for y in ticks], f32)
    for name, (V, tris) in sheets.items():
        rows = np.concatenate([np.concatenate([np.tile(V[list(t)].reshape(1, 9), (len(cols), 1)), cols], 1) for t in tris])
        got = _run(host_exe, "column", rows, tmp_path, np.float64, 2)
        covered = (got[:, 0].astype(int) & 1).reshape(len(tris), len(cols)).sum(0)
        inside = (cols[:, 0] >= 0) & (cols[:, 0] < 2) & (cols[:, 1] >= 0) & (cols[:, 1] < 2)
        assert np.array_equal(covered, inside.astype(int)), name


def _colrange_cases(rng):
    """Rows (lo, hi, m, d, n).  The coordinates of an axis are m + f32(i) * d, i in [0, n)."""
    rows = []

    def axis(m, d, n):
        return f32(m) + np.arange(n, dtype=f32) * f32(d)

    for m, d, n in ((-1.0, 0.0625, 32), (-0.97, 0.031, 96), (0.3, 0.7, 5), (1e6, 0.37, 400), (-3e6, 1.5, 64),
                    (1e6, 1e-3, 2000), (4096.0, 2.0 ** -13, 3000), (65536.0, 1e-4, 257)):   # (the last three: neighbours repeat)
        xs = axis(m, d, n)
        span = float(xs[-1]) - float(xs[0])
        lo = rng.uniform(xs[0] - 0.2 * span, xs[-1] + 0.2 * span, 40)
        hi = lo + rng.uniform(0, 0.5 * span, 40) * rng.integers(0, 2, 40)        # (half of them lo == hi)
        rows += [(a, b, m, d, n) for a, b in zip(lo, hi)]
        pick = xs[rng.integers(0, n, 30)]                                          # exactly on a coordinate
        rows += [(a, a, m, d, n) for a in pick[:10]]
        rows += [(a, xs[-1], m, d, n) for a in pick[10:20]] + [(xs[0], a, m, d, n) for a in pick[20:]]
        rows += [(np.nextafter(a, f32(np.inf)), np.nextafter(b, f32(-np.inf)), m, d, n) for a, b in zip(pick[:10], pick[10:20])]
        rows += [(xs[0] - 3 * span - 1, xs[0] - span - 1, m, d, n), (xs[-1] + span + 1, xs[-1] + 3 * span + 1, m, d, n),   # left, right
                 (np.nextafter(xs[0], f32(-np.inf)), np.nextafter(xs[0], f32(-np.inf)), m, d, n), (xs[0] - 1, xs[-1] + 1, m, d, n)]
        k = n // 2                                                                 # strictly between two columns
        if xs[k + 1] > np.nextafter(xs[k], f32(np.inf)):
            rows.append((np.nextafter(xs[k], f32(np.inf)), np.nextafter(xs[k + 1], f32(-np.inf)), m, d, n))
    for m, d in ((0.25, 0.5), (-7.0, 0.0), (1e6, 3.0), (2.0, -0.5), (2.0, np.inf), (1e6, 0.0), (0.0, -np.inf), (1.0, np.nan)):
        rows += [(m - 1, m + 1, m, d, 1), (m, m, m, d, 1), (m + 1, m + 2, m, d, 1), (m - 2, m - 1, m, d, 1), (m - 1, m + 1, m, d, 7)]
    return np.array(rows, np.float64).astype(f32)


def test_col_range_matches_every_coordinate(host_exe, tmp_path):
    """col_range (the columns a triangle's xy box is tested against) against the plain statement: compute all n coordinates
    m + f32(i) * d in f32; [i0, i1] is the first and the last index whose coordinate lies in [lo, hi].  An empty interval comes
    back as i0 > i1, at the position the monotone sequence gives: i0 = #(coordinates < lo), i1 = #(coordinates <= hi) - 1.
    A spacing that is zero, negative, infinite or NaN gives the whole range, as the header states."""
    rows = _colrange_cases(np.random.default_rng(23))
    got = _run(host_exe, "colrange", rows, tmp_path, np.int32, 2)
    assert len(got) == len(rows)
    kinds = {"empty": 0, "whole": 0, "repeats": 0, "on_coordinate": 0}
    for (lo, hi, m, d, nf), (i0, i1) in zip(rows, got):
        n = int(nf)
        if not (d > 0) or not np.isfinite(d):
            assert (i0, i1) == (0, n - 1), (lo, hi, m, d, n, i0, i1)
            kinds["whole"] += 1
            continue
        xs = f32(m) + np.arange(n, dtype=f32) * f32(d)
        assert np.all(np.diff(xs) >= 0)
        inside = np.nonzero((xs >= lo) & (xs <= hi))[0]
        if len(inside):
            assert (i0, i1) == (inside[0], inside[-1]), (lo, hi, m, d, n, i0, i1, inside[0], inside[-1])
            kinds["on_coordinate"] += int(xs[i0] == lo or xs[i1] == hi)
            kinds["repeats"] += int(np.any(np.diff(xs[i0:i1 + 1]) == 0))
        else:
            assert i0 > i1, (lo, hi, m, d, n, i0, i1)
            kinds["empty"] += 1
        assert (i0, i1) == (np.count_nonzero(xs < lo), np.count_nonzero(xs <= hi) - 1), (lo, hi, m, d, n, i0, i1)
    assert min(kinds.values()) >= 20, kinds
