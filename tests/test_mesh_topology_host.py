"""CPU check of the mesh-topology decisions (sdfkit_amd/csrc/trimesh_topology.h, the functions the kernels of
lib_trimesh_topology.hip call, built with g++ by tests/cpp/mesh_topology_host.cpp) against the numpy model
(tests/mesh_topology_model.py): labels, component rows, census and selection on every small shape and on shuffled meshes, the class
of every (m, f) pair, the sort's digit mask, the host's derived quantities.  Then the model itself: the numbers of the hand-made
shapes, its agreement with a plain union-find, and the invariants any mesh obeys."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_topology_cases as Cs
from tests import mesh_topology_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32, i64, u64 = np.int32, np.int64, np.uint64

MESHES = dict(Cs.SMALL)
MESHES.update({"zigzag_257": lambda: Cs.zigzag(257), "zigzag_685_permuted": lambda: Cs.permuted(*Cs.zigzag(685), 1),
               "tetrahedra_60": lambda: Cs.tetrahedra(60, seed=4), "patch_permuted": lambda: Cs.permuted(*Cs.patch(17, 9), 8),
               "strip_2000_permuted": lambda: Cs.permuted(*Cs.quad_strip(2000), 5)})


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_topology") / "mesh_topology_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cpp", "mesh_topology_host.cpp"),
                           "-o", exe])
    return exe


def _run(exe, mode, blob, tmp_path, dtype):
    src, dst = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
    with open(src, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "mesh topology ok" in p.stdout, (p.returncode, p.stderr)
    return np.fromfile(dst, dtype)


def _keep(count, name):
    return (np.random.default_rng(len(name)).random(count) < 0.6) if count > 2 else np.array(Cs.keep_pattern(count), bool)


@pytest.mark.parametrize("name", list(MESHES))
def test_header_matches_model(host_exe, tmp_path, name):
    V, T = MESHES[name]()
    want = M.topology(V, T)
    keep = _keep(want.count, name)
    blob = struct.pack("<3q", len(V), len(T), want.count) + np.ascontiguousarray(T, i32).tobytes() + M.area_weights(V, T).astype(i64).tobytes() + \
        keep.astype(np.uint8).tobytes()
    out = _run(host_exe, "topology", blob, tmp_path, i64)
    nv, nt, C = len(V), len(T), want.count
    assert out[0] == C and 1 <= out[1] <= nv + 1
    o = 3
    assert np.array_equal(out[o:o + nv], want.vertex); o += nv
    assert np.array_equal(out[o:o + nt], want.triangle); o += nt
    assert np.array_equal(out[o:o + 8 * C].reshape(C, 8), want.rows); o += 8 * C
    assert np.array_equal(out[o:o + 8], want.census); o += 8
    s = M.select(V, T, keep, topo=want)
    kv, kt = out[o:o + 2]; o += 2
    assert (kv, kt) == (len(s.vertex_index), len(s.triangle_index))
    assert np.array_equal(out[o:o + kv], s.vertex_index); o += kv
    assert np.array_equal(out[o:o + kt], s.triangle_index); o += kt
    assert np.array_equal(out[o:], s.triangles) and len(out) == o + 3 * kt


def test_edge_class_of_every_small_pair(host_exe, tmp_path):
    pairs = np.array([(m, f) for m in range(1, 12) for f in range(m + 1)] + [(2 ** 31, 5), (2 ** 32 - 1, 0), (2 ** 32 - 2, 1)], np.uint32)
    out = _run(host_exe, "class", pairs.tobytes(), tmp_path, u64).reshape(-1, 2)
    m, f = pairs[:, 0].astype(i64), pairs[:, 1].astype(i64)
    b, nm, odd, inc = m == 1, m >= 3, m % 2 == 1, (m == 2) & (f != 1)
    assert np.array_equal(out[:, 0], b * 1 + nm * 2 + odd * 4 + inc * 8)
    assert np.array_equal(out[:, 1], 1 + (b.astype(i64) << 8) + (nm.astype(i64) << 16) + (odd.astype(i64) << 24) + (inc.astype(i64) << 32))
    # 64 lanes of the same class sum within their bytes
    assert 64 * 0x0101010101 < 1 << 40 and all(((64 * int(p)) >> (8 * k)) & 255 in (0, 64) for p in out[:, 1] for k in range(5))


def test_sort_mask_covers_exactly_the_bytes_nv_can_set(host_exe, tmp_path):
    nvs = np.array([1, 2, 255, 256, 257, 65535, 65536, 65537, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1], i64)
    out = _run(host_exe, "mask", nvs.tobytes(), tmp_path, np.uint32).reshape(-1, 2)
    for nv, (nbytes, mask) in zip(nvs.tolist(), out.tolist()):
        top = nv - 1
        assert nbytes == (top.bit_length() + 7) // 8
        assert mask == sum(1 << d | 1 << (d + 4) for d in range(nbytes))   # those bytes of the low half (max) and of the high half (min)
        assert top < 1 << 8 * nbytes                                        # no key of the mesh has a bit outside the sorted bytes


def test_derived_quantities_and_size_rules(host_exe, tmp_path):
    rng = np.random.default_rng(2)
    rows = rng.integers(0, 6, (40, 8)).astype(i64)
    rows[:, 7] = rng.integers(0, 3, 40) * (1 << 32) + rng.integers(0, 3, 40)
    rows[5] = rows[6]                                   # a full tie
    rows[7, 7], rows[7, 0] = rows[8, 7], rows[8, 0] + 1   # an area tie
    total = int(rows[:, 7].sum())
    for mt, frac in ((0, 0.0), (3, 0.0), (0, 0.03), (2, 0.05), (0, 1.0)):
        out = _run(host_exe, "derive", rows.tobytes() + struct.pack("<qqd", mt, total, frac), tmp_path, i64)
        per = out[:160].reshape(40, 4)
        assert np.array_equal(per[:, 0], [M.euler(r) for r in rows])
        assert np.array_equal(per[:, 1], [M.watertight(r) for r in rows]) and np.array_equal(per[:, 2], [M.oriented(r) for r in rows])
        assert np.array_equal(per[:, 3].astype(bool), M.keep_small_removed(rows, mt, frac))
        larger = out[160:].reshape(40, 40)
        best = 0
        for c in range(1, 40):
            if larger[c, best]:
                best = c
        assert best == M.largest(rows)
    assert M.largest(np.zeros((0, 8), i64)) == -1


# ---- the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.EXPECTED))
def test_model_reproduces_the_hand_made_shapes(name):
    V, T = Cs.SMALL[name]()
    t = M.topology(V, T)
    assert t.count == 1 and tuple(int(x) for x in t.rows[0][:7]) == Cs.EXPECTED[name]
    chi = {"tetrahedron": 2, "torus_6x5": 0, "moebius_8": 0}
    if name in chi:
        assert M.euler(t.rows[0]) == chi[name]
    if name == "patch_5x3":
        assert int(t.rows[0][3]) == 2 * (5 + 3)   # the perimeter


def test_model_numbers_by_root_and_skips_degenerates():
    V, T = Cs.two_tetrahedra_out_of_order()
    t = M.topology(V, T)
    assert t.vertex.tolist() == [0, 0, 0, 0, -1, 1, 1, 1, 1] and t.triangle.tolist() == [1] * 4 + [0] * 4
    V, T = Cs.with_degenerates()
    t = M.topology(V, T)
    assert t.vertex.tolist() == [0, 0, 0, -1, -1] and t.triangle.tolist() == [0, -1, -1]
    assert int(t.census[7]) == 2 and t.rows[0][:7].tolist() == [1, 3, 3, 3, 0, 3, 0]
    V, T = Cs.no_area()
    assert np.all(M.topology(V, T).rows[:, 7] == 0)


@pytest.mark.parametrize("name", list(MESHES))
def test_model_agrees_with_union_find_and_obeys_invariants(name):
    V, T = MESHES[name]()
    t = M.topology(V, T)
    uv, ut, uc = M.labels_union_find(len(V), T)
    assert uc == t.count and np.array_equal(uv, t.vertex) and np.array_equal(ut, t.triangle)
    r = t.rows
    assert np.array_equal(r.sum(axis=0)[1:7], t.census[1:7]) and int(r[:, 0].sum()) == len(T) - int(t.census[7])
    assert int(r[:, 7].sum()) == int(M.area_weights(V, T)[t.triangle >= 0].sum())
    keys, m, f = M.edges(T)
    assert int(m.sum()) == 3 * int(r[:, 0].sum()) and np.all(f <= m)          # every live triangle gives three edge uses
    assert np.all(r[:, 3] <= r[:, 5]) and np.all(r[:, 5] <= r[:, 3] + r[:, 4])   # boundary edges are odd; odd ones are boundary or non-manifold
    assert np.all((r[:, 5] % 2) == (r[:, 0] % 2))                              # sum of m = 3 F, so the odd edges have F's parity
    # numbering by ascending root: the first vertex of component c comes before that of c + 1
    firsts = [int(np.flatnonzero(t.vertex == c)[0]) for c in range(t.count)]
    assert firsts == sorted(firsts)
    # a selection is a mesh whose own topology is the kept rows
    keep = _keep(t.count, name)
    s = M.select(V, T, keep, topo=t)
    if len(s.triangle_index):
        t2 = M.topology(s.vertices, s.triangles)
        assert t2.count == int(keep.sum()) and np.array_equal(t2.rows[:, :7], r[keep][:, :7]) and int(t2.census[7]) == 0


def test_recorded_cases_are_what_the_model_gives_today():
    doc = Cs.load()
    assert [c["mesh"] for c in doc["cases"]] == Cs.RECORDED
    assert doc["cases"] == [Cs.record(n) for n in Cs.RECORDED]
    assert os.path.getsize(Cs.FIXTURE) < 64 << 10
