"""CPU check of the welding decisions (sdfkit_amd/csrc/trimesh_weld.h, the functions the kernels of lib_trimesh_weld.hip call, built
with g++ by tests/cpp/mesh_weld_host.cpp and run one item at a time in the kernels' order) against the numpy model
(tests/mesh_weld_model.py): every case of tests/mesh_weld_cases.py under the four flag combinations, the canonical key, the pass
mask at every byte, the keep rules, the lattice key at cell faces, the span refusal.  Then the model itself: the invariants any
weld obeys, on random soups."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_weld_cases as Cs
from tests import mesh_weld_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, i32, i64, u32, u64 = np.float32, np.float64, np.int32, np.int64, np.uint32, np.uint64

MESHES = dict(Cs.SMALL)
MESHES.update({f"sized_{n}": (lambda n=n: Cs._plain(Cs.sized(n))) for n in Cs.SIZES})
MESHES.update({"big_permuted_soup": lambda: Cs._plain(Cs.big_permuted_soup()),
               "torus_soup_permuted_lattice": lambda: Cs._plain(Cs.permuted(*Cs.soup(*Cs.torus()), 3), tolerance=0.125)})


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_weld") / "mesh_weld_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cpp", "mesh_weld_host.cpp"), "-o", exe])
    return exe


def _run(exe, mode, blob, tmp_path, dtype):
    src, dst = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
    with open(src, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "mesh weld ok" in p.stdout, (p.returncode, p.stderr)
    return np.fromfile(dst, dtype)


def _weld(exe, tmp_path, V, T, tol, flags):
    blob = struct.pack("<3q2f", len(V), len(T), flags, tol, 0.0) + M.bits(V).tobytes() + np.ascontiguousarray(T, i32).tobytes()
    return _run(exe, "weld", blob, tmp_path, i64)


def _check(out, want, nv, passes, what):
    assert out[0] == 0 and out[1] == passes and out[2] == want.groups, what
    kv, kt = int(out[3]), int(out[4])
    assert (kv, kt) == (len(want.vertex_index), len(want.triangle_index)), what
    o = 5
    assert np.array_equal(out[o:o + nv], want.vertex_map), what; o += nv
    assert np.array_equal(out[o:o + kv], want.vertex_index), what; o += kv
    assert np.array_equal(out[o:o + kt], want.triangle_index), what; o += kt
    assert np.array_equal(out[o:], want.triangles) and len(out) == o + 3 * kt, what


@pytest.mark.parametrize("name", list(MESHES))
def test_header_matches_model(host_exe, tmp_path, name):
    V, T, _, tol = MESHES[name]()
    for flags in Cs.FLAGS:
        _check(_weld(host_exe, tmp_path, V, T, tol, flags), M.weld(V, T, None, tol, flags), len(V), M.passes(V, tol), (name, flags))


def test_canonical_key_zeros_subnormals_and_single_axis_differences(host_exe, tmp_path):
    z, sub, sub2 = f32(-0.0), np.nextafter(f32(0), f32(1)), np.nextafter(f32(0), f32(-1))
    pairs = [((0, 0, 0), (z, z, z), True), ((z, 1, 2), (0, 1, 2), True), ((1, z, 2), (1, 0, 2), True), ((1, 2, z), (1, 2, 0), True),
             ((sub, 0, 0), (0, 0, 0), False), ((sub, 0, 0), (sub2, 0, 0), False), ((sub, sub, sub), (sub, sub, sub), True),
             ((1, 2, 3), (1, 2, 4), False), ((1, 2, 3), (1, 5, 3), False), ((1, 2, 3), (6, 2, 3), False), ((1, 2, 3), (1, 2, 3), True),
             ((1, 2, 3), (np.nextafter(f32(1), f32(2)), 2, 3), False), ((-1, 2, 3), (1, 2, 3), False)]
    P = np.array([[p, q] for p, q, _ in pairs], f32)
    out = _run(host_exe, "keys", M.bits(P).tobytes(), tmp_path, u64).reshape(-1, 3)
    assert out[:, 2].astype(bool).tolist() == [s for _, _, s in pairs]
    c = M.canonical(P[:, 0]).astype(u64)
    assert np.array_equal(out[:, 0], c[:, 0]) and np.array_equal(out[:, 1], c[:, 2] << u64(32) | c[:, 1])
    # the two keys together are the whole position: equal keys <=> equal as values
    q = M.canonical(P[:, 1]).astype(u64)
    same = (c[:, 0] == q[:, 0]) & ((c[:, 2] << u64(32) | c[:, 1]) == (q[:, 2] << u64(32) | q[:, 1]))
    assert same.tolist() == [s for _, _, s in pairs]
    assert np.array_equal(same, np.all(P[:, 0] == P[:, 1], axis=1))


def test_pass_mask_at_every_byte_position(host_exe, tmp_path):
    diffs = [0] + [1 << b for b in range(64)] + [0xff << (8 * d) for d in range(8)] + [(1 << 63) | 1, 0x0000010000000100, 2 ** 64 - 1]
    out = _run(host_exe, "mask", np.array(diffs, u64).tobytes(), tmp_path, u32).reshape(-1, 2)
    for d, (mask, n) in zip(diffs, out.tolist()):
        assert mask == M.pass_mask(d) == sum(1 << k for k in range(8) if (d >> (8 * k)) & 255) and n == bin(mask).count("1")
    assert out[0].tolist() == [0, 0] and [m for m, _ in out[1:65].tolist()] == [1 << (b // 8) for b in range(64)]


def test_ordered_bits_order_as_the_values_do(host_exe, tmp_path):
    vals = np.sort(np.concatenate([np.random.default_rng(0).standard_normal(200).astype(f32) * f32(1e3), np.array(
        [0.0, 1e-45, -1e-45, 1e-38, -1e-38, 3.4e38, -3.4e38, 4096, -8192], f32)]))
    vals = np.concatenate([vals[vals < 0], np.array([-0.0, 0.0], f32), vals[vals > 0]])
    out = _run(host_exe, "ordered", M.bits(vals).tobytes(), tmp_path, u32).reshape(-1, 2)
    assert np.all(np.diff(out[:, 0].astype(i64)) > 0) and np.array_equal(out[:, 1], M.bits(vals))


def test_keep_rules_under_all_four_flag_combinations(host_exe, tmp_path):
    rows = [(a, b, c, v, r, u, fl) for (a, b, c) in ((0, 1, 2), (0, 0, 1), (0, 1, 1), (2, 1, 2), (3, 3, 3)) for (v, r) in ((4, 4), (4, 2))
            for u in (0, 1) for fl in (0, 1, 2, 3, 4, 7, -1)]
    out = _run(host_exe, "keep", np.array(rows, i32).tobytes(), tmp_path, i32).reshape(-1, 4)
    for (a, b, c, v, r, u, fl), (kt, kv, ok, mp) in zip(rows, out.tolist()):
        deg = a == b or b == c or a == c
        assert bool(kt) == (bool(fl & 1) or not deg)
        assert bool(kv) == (r == v and (bool(u) or bool(fl & 2)))
        assert bool(ok) == (fl in (0, 1, 2, 3)) and mp == (5 if u else -1)


def _lattice(exe, tmp_path, tol, P):
    P = np.asarray(P, f32).reshape(-1, 3)
    blob = struct.pack("<7f", tol, *P.min(axis=0), *P.max(axis=0)) + M.bits(P).tobytes()
    return _run(exe, "lattice", blob, tmp_path, i64)


@pytest.mark.parametrize("tol", [0.25, 0.1, 1e-3, 3.0])
def test_lattice_key_at_cell_faces(host_exe, tmp_path, tol):
    """p = k tol exactly (as f32) and one ulp below: the model's binary64 floor decides, and the header decides the same."""
    t = f32(tol)
    k = np.array([-7, -1, 0, 1, 2, 5, 100], f64)
    face = (k * f64(t)).astype(f32)
    x = np.concatenate([face, np.nextafter(face, f32(-np.inf)), np.nextafter(face, f32(np.inf))])
    P = np.stack([x, x[::-1], np.roll(x, 3)], 1)
    out = _lattice(host_exe, tmp_path, t, P)
    c = M.cells(P, t)
    assert out[0] == 1 and out[1] == 1
    assert np.array_equal(out[3:], c[:, 2] << 42 | c[:, 1] << 21 | c[:, 0])
    assert M.pass_mask(int(np.bitwise_or.reduce(out[3:] ^ out[3]))) & ~int(out[2]) == 0     # the passes skipped by span hold no difference
    if tol == 0.25:   # a power of two: the face is exact, the point on it belongs to the upper cell
        assert np.array_equal(c[:7, 0] - c[7:14, 0], np.ones(7, i64)) and np.array_equal(c[:7, 0], c[14:, 0])


def test_span_refusal_at_two_to_the_21_cells(host_exe, tmp_path):
    ok = np.array([(0, 0, 0), (2 ** 21 - 1, 0.5, -3)], f32)
    bad = np.array([(0, 0, 0), (2 ** 21, 0.5, -3)], f32)
    assert _lattice(host_exe, tmp_path, 1.0, ok)[0] == 1 and _lattice(host_exe, tmp_path, 1.0, bad)[0] == 0
    assert _lattice(host_exe, tmp_path, 1.0, ok[:, ::-1])[0] == 1 and _lattice(host_exe, tmp_path, 1.0, bad[:, ::-1])[0] == 0
    M.cells(ok, 1.0)
    with pytest.raises(M.Refused):
        M.cells(bad, 1.0)
    T = np.array([(0, 1, 1)], i32)
    assert _weld(host_exe, tmp_path, ok, T, 1.0, 0)[0] == 0 and _weld(host_exe, tmp_path, bad, T, 1.0, 0).tolist() == [1]
    assert _weld(host_exe, tmp_path, bad, T, 0.0, 0)[0] == 0                              # exact mode has no span
    for tol in (-1.0, np.nan, np.inf):
        assert _weld(host_exe, tmp_path, ok, T, tol, 0).tolist() == [1]
        assert _lattice(host_exe, tmp_path, tol, ok)[1] == 0
        with pytest.raises(M.Refused):
            M.weld(ok, T, None, tol)
    assert _weld(host_exe, tmp_path, ok, T, 0.0, 4).tolist() == [1]
    with pytest.raises(M.Refused):
        M.weld(ok, T, None, 0.0, 4)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _random_soup(seed):
    rng = np.random.default_rng(seed)
    V, T = Cs.permuted(*Cs.soup(*Cs.patch(3 + seed % 5, 2 + seed % 3)), seed)
    extra = rng.integers(0, len(V), (4, 3)).astype(i32)                       # triangles between arbitrary soup vertices
    return V, np.concatenate([T, extra, np.array([(1, 1, 2)], i32)])


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("tol", [0.0, 0.125])
def test_model_invariants_on_random_soups(seed, tol):
    V, T = _random_soup(seed)
    cols = Cs.index_colors(len(V))
    for flags in Cs.FLAGS:
        w = M.weld(V, T, cols, tol, flags)
        assert np.array_equal(M.bits(w.vertices), M.bits(V[w.vertex_index])) and np.array_equal(M.bits(w.colors), M.bits(cols[w.vertex_index]))
        assert np.array_equal(w.triangles.reshape(-1, 3), w.vertex_map[T[w.triangle_index]])           # every kept triangle is the map of its old one
        assert np.all(w.rep <= np.arange(len(V))) and np.array_equal(w.rep[w.rep], w.rep)
        assert np.all(np.diff(w.vertex_index) > 0) and np.all(np.diff(w.triangle_index) > 0)
        assert w.merged + w.unreferenced + len(w.vertex_index) == len(V) and w.degenerate + len(w.triangle_index) == len(T)
        if not flags & 1:
            assert not np.any(M.degenerate(w.triangles.reshape(-1, 3)))
        if not flags & 2:
            assert np.array_equal(np.unique(w.triangles), np.arange(len(w.vertex_index)))
        # idempotence: welding the welded mesh is the identity
        again = M.weld(w.vertices, w.triangles, w.colors, tol, flags)
        assert np.array_equal(again.vertex_map, np.arange(len(w.vertex_index))) and again.merged == 0 and again.unreferenced == 0
        assert np.array_equal(again.triangles, w.triangles) and np.array_equal(M.bits(again.vertices), M.bits(w.vertices))
        assert again.degenerate == 0
    if tol == 0:   # the soup of a patch welds back to the patch's vertex count
        qx, qy = 3 + seed % 5, 2 + seed % 3
        assert len(M.weld(V, T[:-5]).vertex_index) == (qx + 1) * (qy + 1)


@pytest.mark.parametrize("name", ["tetrahedron", "torus", "patch", "zigzag"])
def test_model_is_the_identity_on_a_clean_mesh(name):
    V, T = {"tetrahedron": Cs.tetrahedron, "torus": Cs.torus, "patch": lambda: Cs.permuted(*Cs.patch(6, 4), 1), "zigzag": lambda: Cs.zigzag(300)}[name]()
    for tol in (0.0, 1e-3):
        w = M.weld(V, T, None, tol)
        assert np.array_equal(w.vertex_map, np.arange(len(V))) and np.array_equal(w.triangles.reshape(-1, 3), T)
        assert np.array_equal(M.bits(w.vertices), M.bits(V)) and (w.merged, w.degenerate, w.unreferenced) == (0, 0, 0)


def test_model_numbers_of_the_hand_made_cases():
    got = {n: M.weld(*Cs.SMALL[n]()[:2], None, Cs.SMALL[n]()[3]) for n in Cs.SMALL}
    assert (len(got["tetrahedron_soup"].vertex_index), got["tetrahedron_soup"].merged) == (4, 8)
    assert (len(got["cube_soup"].vertex_index), len(got["cube_soup"].triangle_index)) == (8, 12)
    assert got["one_coordinate_pairs"].rep.tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    assert got["signed_zeros"].rep.tolist() == [0, 1, 2, 0, 1, 2, 6]
    a = got["all_equal"]
    assert (len(a.vertex_index), len(a.triangle_index), a.merged, a.degenerate, a.unreferenced) == (0, 0, 4, 2, 1) and np.all(a.vertex_map == -1)
    assert got["first_and_last"].rep.tolist() == [0, 1, 2, 3, 0]
    u = got["unreferenced_and_degenerate"]
    assert (u.merged, u.degenerate, u.unreferenced) == (1, 3, 3) and u.vertex_map.tolist() == [0, 1, 2, -1, -1, 1, -1]
    assert len(got["jittered_lattice"].vertex_index) == 8 * 6 and got["jittered_lattice"].merged == 3 * 70 - 48
    assert len(got["straddling_pair_lattice"].vertex_index) == 4 and got["straddling_pair_lattice"].merged == 0
    assert len(got["strip_soup_tiny"].vertex_index) == 40 and len(got["cube_soup_moved"].vertex_index) == 8
    V, T, cols, _ = Cs.SMALL["torus_soup_colored"]()
    w = M.weld(V, T, cols)
    assert len(w.vertex_index) == 30 and np.array_equal(M.bits(w.colors), M.bits(cols[w.rep[w.vertex_index]]))
    # exact mode: x needs its passes, (z, y) theirs; a clean unit tetrahedron differs in the top bytes only
    assert M.passes(*Cs.tetrahedron()[:1], 0.0) == 2 + 4


def test_recorded_cases_are_what_the_model_gives_today():
    doc = Cs.load()
    assert [c["mesh"] for c in doc["cases"]] == Cs.RECORDED
    assert doc["cases"] == [Cs.record(n) for n in Cs.RECORDED]
    assert os.path.getsize(Cs.FIXTURE) < 64 << 10
