"""What the simplification stress cases (tests/mesh_simplify_stress_cases.py) are there for, proved on the CPU from the numpy model
(tests/mesh_simplify_model.py) alone, before any device sees them:

  * every case has its property: the group sizes, the run lengths and where their lowest index lies, the number of groups, which
    groups are kept, how many fall back and in which lane of which wave of k_ts_place, the exact results of the census;
  * the header (sdfkit_amd/csrc/trimesh_simplify.h, built by tests/cpp/mesh_simplify_host.cpp as tests/test_mesh_simplify_host.py
    builds it) equals the model bit for bit on every case;
  * WRONG VARIANTS: `reference` below restates one group's placement and the triangle rule a second time, item by item in plain
    Python floats (binary64, correctly rounded, never fused), and equals the model bit for bit without a variant.  Every variant
    is one small change to it -- another order, another chunk, a contracted product, a laxer comparison, a sort one byte short --
    and must change an output (float32 bits, integers or stats) on the case NAMED for it in VARIANTS: a library with that mistake
    fails that case.

All variants are caught; none had to be argued away.  The byte-edge cases of 257 and 65 537 groups cannot catch a short sort (the
top byte holds one group there, see byte_edge); those of 256, 65 535 and 65 536 do.

The whole file takes about 17 s on one CPU core, the compile of the host executable (1.5 s) included; no item takes longer than
a second (the slowest: the two groups of 4196 members and 3000 corners through `reference`)."""
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import mesh_simplify_model as M
from tests import mesh_simplify_stress_cases as S
from tests import mesh_weld_model as W
from tests import pointcloud_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, i32, i64, u64 = np.float32, np.float64, np.int32, np.int64, np.uint64


# ---- the cases by name: (case, the (placement, flags) pairs they are about) ------------------------------------------------------
ALL = tuple((p, fl) for p in (0, 1, 2) for fl in (0, 1, 2))
CASES = {}
CASES.update({f"centroid_{n}": (lambda n=n: S.centroid_order(n), ((1, 0), (2, 0), (0, 1))) for n in S.CENTROID_SIZES})
CASES.update({"knife_edge": (S.knife_edge, ((2, 0), (2, 1))), "shared_corners": (S.shared_corners, ALL)})
CASES.update({f"large_{g}": (lambda g=g: S.large_groups(g), ((1, 0), (2, 0), (2, 2))) for g in (65535, 65537)})
CASES.update({"long_runs": (S.long_runs, ((0, 0), (0, 1), (0, 2), (2, 0)))})
CASES.update({f"bytes_{g}": (lambda g=g: S.byte_edge(g), ((0, 0), (2, 2), (1, 1))) for g in S.BYTE_EDGES})
CASES.update({f"triangles_{n}": (lambda n=n: S.many_triangles(n), ((2, 0), (1, 2), (0, 1))) for n in S.TRIANGLE_COUNTS})
CASES.update({f"sheets_{k}": (lambda k=k: S.tiled_sheets(k), ((2, 0), (2, 2), (1, 0))) for k in S.SHEET_TILES})
CASES.update({f"wave_{k}": (lambda k=k: S.one_per_wave(k), ((2, 0), (2, 1))) for k in S.LANE_PATTERNS})
CASES.update({"census": (S.census, ALL)})
CASES.update({f"scaled_{k}": (lambda k=k: S.scaled_corner(k), ((0, 0), (1, 0), (2, 0), (2, 2))) for k in S.SCALES})


def case(name):
    return CASES[name][0]()[:4]


# ---- the second statement of the function, with its wrong variants ---------------------------------------------------------------
def _fma(a, b, c):
    """a b + c rounded once (what a contracted multiply-add gives)."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _mean(rows, variant):
    """rows: the members' float32 triples in ascending index -> the chunked mean per axis (floats)."""
    n = len(rows)
    if variant == "members_descending":
        rows = rows[::-1]
    chunk = {"no_chunking": n, "chunk_64": 64}.get(variant, S.CHUNK)
    zero = f32(0) if variant == "f32_accumulation" else 0.0
    wide = (lambda x: f32(x)) if variant == "f32_accumulation" else float
    total = [zero] * 3
    for i in range(0, n, chunk):
        part = [zero] * 3
        for row in rows[i:i + chunk]:
            part = [part[a] + wide(row[a]) for a in range(3)]
        total = [total[a] + part[a] for a in range(3)]
    if variant == "f32_accumulation":
        return [float(total[a] / f32(n)) for a in range(3)]
    if variant == "reciprocal":
        return [total[a] * (1.0 / n) for a in range(3)]
    return [total[a] / float(n) for a in range(3)]


def _triangle_terms(p, c, variant):
    q = [[float(p[k][a]) - c[a] for a in range(3)] for k in range(3)]
    e1 = [q[1][a] - q[0][a] for a in range(3)]
    e2 = [q[2][a] - q[0][a] for a in range(3)]
    if variant == "contracted_normal":
        cross = lambda a, b: _fma(e1[a], e2[b], -(e1[b] * e2[a]))   # noqa: E731
    else:
        cross = lambda a, b: e1[a] * e2[b] - e1[b] * e2[a]          # noqa: E731
    n = [cross(1, 2), cross(2, 0), cross(0, 1)]
    d = -((n[0] * q[0][0] + n[1] * q[0][1]) + n[2] * q[0][2])
    return [n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2], d * n[0], d * n[1], d * n[2]]


def _jacobi(Q):
    a = [[Q[0], Q[1], Q[2]], [Q[1], Q[3], Q[4]], [Q[2], Q[4], Q[5]]]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(PM.SWEEPS):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            if theta < 0.0:
                t = -t
            cs = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * cs
            a[p][p], a[q][q] = a[p][p] - t * apq, a[q][q] + t * apq
            a[p][q] = a[q][p] = 0.0
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = cs * arp - sn * arq
            a[r][q] = a[q][r] = sn * arp + cs * arq
            for k in range(3):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p], v[k][q] = cs * vkp - sn * vkq, sn * vkp + cs * vkq
    return [a[0][0], a[1][1], a[2][2]], v


def place_group(V, T, cols, cell, placement, members, inc_start, inc, variant=None):
    """trimesh_simplify.h place_group for one group -> (position float32 x 3, colour float32 x 3, fallback, p before the cell test
    or None, the number of eigenpairs that took part)."""
    first = members[0]
    if placement == M.REPRESENTATIVE:
        return V[first].copy(), (cols[first].copy() if cols is not None else np.zeros(3, f32)), False, None, 0
    c = _mean([V[m] for m in members], variant)
    colour = np.array(_mean([cols[m] for m in members], variant), f64).astype(f32) if cols is not None else np.zeros(3, f32)
    if placement == M.CENTROID:
        return np.array(c, f64).astype(f32), colour, False, None, 0
    about = [float(f32(x)) for x in c] if variant == "rounded_centroid" else c
    chunk_size = S.CHUNK
    total = [0.0] * 9
    seen = set()
    for i in range(0, len(members), chunk_size):
        chunk = [0.0] * 9
        for m in members[i:i + chunk_size]:
            own = [0.0] * 9
            corners = [int(e) for e in inc[inc_start[m]:inc_start[m + 1]]]
            if variant == "corners_descending":
                corners = corners[::-1]
            for e in corners:
                if variant == "once_per_group":
                    if e // 3 in seen:
                        continue
                    seen.add(e // 3)
                terms = _triangle_terms(V[T[e // 3]], about, variant)
                if variant == "straight_into_chunk":
                    chunk = [chunk[k] + terms[k] for k in range(9)]
                else:
                    own = [own[k] + terms[k] for k in range(9)]
            chunk = [chunk[k] + own[k] for k in range(9)]
        total = [total[k] + chunk[k] for k in range(9)]
    l, v = _jacobi(total[:6])
    lmax = l[0]
    if variant != "lmax_is_l0":
        lmax = l[1] if l[1] > lmax else lmax
        lmax = l[2] if l[2] > lmax else lmax
    ok, x, took = lmax > 0.0, [0.0] * 3, 0
    if ok:
        cut = float(M.TRUNCATION) * lmax
        nb = [-total[6], -total[7], -total[8]]
        for i in range(3):
            if not (l[i] >= cut if variant == "truncation_ge" else l[i] > cut):
                continue
            took += 1
            s = (v[0][i] * nb[0] + v[1][i] * nb[1]) + v[2][i] * nb[2]
            t = s / l[i] if l[i] != 0.0 else math.copysign(math.inf, s) if s != 0.0 else math.nan
            x = [x[k] + v[k][i] * t for k in range(3)]
    p = [c[a] + x[a] for a in range(3)]
    size = float(f32(cell))
    for a in range(3):
        k = math.floor(float(V[first][a]) / size)
        lo, hi = k * size, (k + 1.0) * size
        ok = ok and math.isfinite(p[a]) and p[a] >= lo and (p[a] <= hi if variant == "closed_upper_face" else p[a] < hi)
    return np.array(p if ok else c, f64).astype(f32), colour, not ok, p, took


def keep_triangles(G, groups, flags, variant=None):
    """G (nt, 3): the corners as group numbers -> the kept triangles' mask: the records, the two radix sorts pass by pass (each a
    stable sort of one byte), the heads, the runs."""
    nt = len(G)
    deg = W.degenerate(G)
    if flags & M.KEEP_DUPLICATES:
        return ~deg
    tri = np.sort(G, axis=1).astype(u64)
    tri[deg] = 0
    lo, mid, hi = tri[:, 0], tri[:, 1], tri[:, 2]
    nb = M.index_bytes(groups)
    order = np.arange(nt)
    for d in range(nb - (variant == "first_sort_short")):
        order = order[np.argsort((lo[order] >> u64(8 * d)) & u64(255), kind="stable")]
    second = nb - (variant == "second_sort_short")
    for key in (mid, hi):                                       # the digits of mid lie below those of hi in the 64-bit key
        for d in range(second):
            order = order[np.argsort((key[order] >> u64(8 * d)) & u64(255), kind="stable")]
    a, b, c = lo[order], mid[order], hi[order]
    same = c[1:] == c[:-1]
    if variant != "same_set_without_mid":
        same &= b[1:] == b[:-1]
    if variant != "same_set_without_lo":
        same &= a[1:] == a[:-1]
    head = np.r_[True, ~same] if nt else np.zeros(0, bool)
    start = np.flatnonzero(head)
    length = np.diff(np.r_[start, nt])
    pick = start + length - 1 if variant == "last_of_run" else start
    keep = c[pick] != 0
    if flags & M.CANCEL_PAIRS:
        keep &= (length < 2) if variant == "cancel_two_or_more" else (length % 2 == 1)
    out = np.zeros(nt, bool)
    out[order[pick[keep]]] = True
    return out


def reference(V, T, cols, cell, placement, flags, variant=None, only=None):
    """The outputs of sdfk_trimesh_simplify from place_group and keep_triangles; the groups themselves are the model's.
    only: the old indices of representatives -- place these groups alone (the others' rows stay zero)."""
    s = M.simplify(V, T, cols, cell, 0, M.KEEP_DUPLICATES)
    rep, groups = s.rep, s.groups
    is_rep = rep == np.arange(len(V))
    gnum = np.cumsum(is_rep) - is_rep
    tkeep = keep_triangles(gnum[rep[T]], groups, flags, variant)
    used = np.zeros(len(V), bool)
    used[rep[T[tkeep]].reshape(-1)] = True
    vkeep = is_rep & used
    vertex_index = np.flatnonzero(vkeep)
    inc_start, inc = M.corner_lists(len(V), T)
    order = np.argsort(rep, kind="stable")
    bounds = np.r_[np.flatnonzero(np.r_[True, rep[order][1:] != rep[order][:-1]]), len(V)]
    members_of = {int(rep[order[b]]): order[b:e].tolist() for b, e in zip(bounds[:-1], bounds[1:])}
    pos, col = np.zeros((len(vertex_index), 3), f32), np.zeros((len(vertex_index), 3), f32)
    fallback, before, took = np.zeros(len(vertex_index), bool), {}, {}
    for o, r in enumerate(vertex_index.tolist()):
        if only is not None and r not in only:
            continue
        pos[o], col[o], fallback[o], before[r], took[r] = place_group(V, T, cols, cell, placement, members_of[r], inc_start, inc, variant)
    count = int(fallback.sum())
    if variant == "fallbacks_over_all_groups":
        count = sum(place_group(V, T, cols, cell, placement, m, inc_start, inc)[2] for m in members_of.values())
    return {"triangle_index": np.flatnonzero(tkeep), "vertex_index": vertex_index, "vertices": pos, "colors": col, "fallbacks": count,
            "fallback": fallback, "before": before, "took": took, "rep": rep, "groups": groups, "members": members_of}


def _differs(a, b):
    return not (np.array_equal(a["triangle_index"], b["triangle_index"]) and np.array_equal(a["vertex_index"], b["vertex_index"])
                and np.array_equal(W.bits(a["vertices"]), W.bits(b["vertices"])) and np.array_equal(W.bits(a["colors"]), W.bits(b["colors"]))
                and a["fallbacks"] == b["fallbacks"])


def _equals_model(ref, want):
    return (np.array_equal(ref["triangle_index"], want.triangle_index) and np.array_equal(ref["vertex_index"], want.vertex_index)
            and np.array_equal(W.bits(ref["vertices"]), W.bits(want.vertices)) and np.array_equal(W.bits(ref["colors"]), W.bits(want.colors))
            and ref["fallbacks"] == want.fallbacks)


SMALL = [n for n in CASES if not n.startswith("large_")]


@pytest.mark.parametrize("name", SMALL)
def test_reference_without_a_variant_is_the_model(name):
    V, T, cols, cell = case(name)
    for placement, flags in CASES[name][1]:
        assert _equals_model(reference(V, T, cols, cell, placement, flags), M.simplify(V, T, cols, cell, placement, flags)), (name, placement, flags)


# variant -> (the case that catches it, placement, flags)
VARIANTS = {
    "members_descending": ("centroid_31", 1, 0), "no_chunking": ("centroid_65", 1, 0), "chunk_64": ("centroid_65", 1, 0),
    "f32_accumulation": ("centroid_32", 1, 0), "reciprocal": ("centroid_31", 1, 0),
    "corners_descending": ("knife_edge", 2, 0), "contracted_normal": ("knife_edge", 2, 0), "rounded_centroid": ("knife_edge", 2, 0),
    "once_per_group": ("shared_corners", 2, 0), "straight_into_chunk": ("knife_edge", 2, 0),
    "truncation_ge": ("census", 2, 0), "lmax_is_l0": ("census", 2, 0), "closed_upper_face": ("census", 2, 0),
    "same_set_without_lo": ("long_runs", 0, 0), "same_set_without_mid": ("long_runs", 0, 0), "last_of_run": ("long_runs", 0, 0),
    "cancel_two_or_more": ("long_runs", 0, 2), "first_sort_short": ("bytes_65536", 0, 0), "second_sort_short": ("bytes_65536", 0, 0),
    "fallbacks_over_all_groups": ("census", 2, 0),
}
# the other cases that must catch a variant too: every centroid size its order, both sides of a byte its sorts
ALSO = [("members_descending", "centroid_32", 1, 0), ("members_descending", "centroid_33", 1, 0), ("members_descending", "centroid_65", 1, 0),
        ("f32_accumulation", "centroid_31", 1, 0), ("f32_accumulation", "centroid_33", 1, 0),
        ("first_sort_short", "bytes_256", 0, 0), ("second_sort_short", "bytes_256", 0, 0), ("first_sort_short", "bytes_65535", 0, 0),
        ("second_sort_short", "bytes_65535", 0, 0), ("first_sort_short", "bytes_255", 0, 0),
        ("cancel_two_or_more", "triangles_2049", 0, 2), ("last_of_run", "triangles_257", 0, 0), ("fallbacks_over_all_groups", "sheets_64", 2, 2)]


@pytest.mark.parametrize("variant,name,placement,flags", [(v,) + VARIANTS[v] for v in VARIANTS] + ALSO)
def test_a_wrong_variant_is_caught_by_its_case(variant, name, placement, flags):
    V, T, cols, cell = case(name)
    true = reference(V, T, cols, cell, placement, flags)
    assert _equals_model(true, M.simplify(V, T, cols, cell, placement, flags))
    assert _differs(reference(V, T, cols, cell, placement, flags, variant), true), (variant, name)


def test_which_outputs_the_order_variants_move():
    """Not only that, but where: on centroid_65 the x of the group is moved by the members' order, its y by the chunking."""
    V, T, cols, cell = case("centroid_65")
    true = reference(V, T, cols, cell, 1, 0)
    moved = lambda v: (W.bits(reference(V, T, cols, cell, 1, 0, v)["vertices"])[0] != W.bits(true["vertices"])[0]).tolist()   # noqa: E731
    assert moved("members_descending")[0] and moved("no_chunking") == [False, True, False] and moved("chunk_64") == [False, True, False]
    assert (W.bits(reference(V, T, cols, cell, 1, 0, "no_chunking")["colors"])[0] != W.bits(true["colors"])[0]).tolist() == [True, False, False]


# ---- every case has its property -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.CENTROID_SIZES)
def test_centroid_cases_sit_beside_a_float32_midpoint(n):
    V, T, cols, cell = S.centroid_order(n)
    s = M.simplify(V, T, cols, cell, 1, 0)
    assert s.groups == 3 and np.bincount(s.rep).max() == n and s.rep[n - 1] == 0 and len(s.vertex_index) == 3
    k = 8 if n <= S.CHUNK + 1 else 16
    for axis, (odd, count, tiny) in enumerate(((1, k, S.TINY), (1, k, S.TINY), (1, 1, 2.0 ** -49) if n == 31 else (3, 0, 0.0))):
        col = V[:n, axis]
        assert col.max() / col[col > 0].min() > 2 ** 29 or count == 0
        mean = sum(Fraction(float(x)) for x in col) / n
        midpoint = Fraction(1, 2) + Fraction(odd, 2 ** 25)                # between two neighbouring float32 values of [1/2, 1)
        assert mean - midpoint == Fraction(tiny) * count / n and mean - midpoint < Fraction(1, 2 ** 52)   # on it, or within two ulps above
        assert not np.all(np.diff(col) > 0)
    # the sums are inexact: a TINY member is below half an ulp of the running sum it is added to in the wrong orders
    assert S.TINY < np.spacing(f64(8.0)) / 2


def test_knife_edge_and_shared_corners():
    V, T, cols, cell = S.knife_edge()
    r = reference(V, T, cols, cell, 2, 0)
    inc_start, inc = M.corner_lists(len(V), T)
    sides = []
    for i in range(S.KNIFE_GROUPS):
        first = i * (S.KNIFE_MEMBERS + 2 * S.KNIFE_CORNERS * S.KNIFE_MEMBERS)
        members = r["members"][first]
        assert len(members) == S.KNIFE_MEMBERS > S.CHUNK and r["took"][first] == 3
        P = np.array([64 * i + 16, 8, 8], i64)                                               # in sixteenths
        for m in members:
            assert inc_start[m + 1] - inc_start[m] == S.KNIFE_CORNERS
            for e in inc[inc_start[m]:inc_start[m + 1]]:
                a, b, c = (np.round(V[T[e // 3]].astype(f64) * 16).astype(i64) - P).tolist()
                assert np.array_equal(V[T[e // 3]].astype(f64) * 16, np.round(V[T[e // 3]].astype(f64) * 16))
                det = a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0])
                assert det == 0                                                                  # the plane passes through P, exactly
        p = r["before"][first]
        assert abs(p[0] - (4 * i + 1)) < 2.0 ** -40 and abs(p[1] - 0.5) < 2.0 ** -40 and abs(p[2] - 0.5) < 2.0 ** -40
        o = np.searchsorted(r["vertex_index"], first)
        assert r["fallback"][o] == (p[0] >= 4 * i + 1)
        sides.append(bool(r["fallback"][o]))
    assert 1 <= sum(sides) <= S.KNIFE_GROUPS - 1, sides                                       # both sides of the face occur
    for variant, moved in S.KNIFE_MOVED_BY.items():
        w = reference(V, T, cols, cell, 2, 0, variant)
        firsts = [i * (S.KNIFE_MEMBERS + 2 * S.KNIFE_CORNERS * S.KNIFE_MEMBERS) for i in moved]
        assert all(w["fallback"][np.searchsorted(w["vertex_index"], f)] != r["fallback"][np.searchsorted(r["vertex_index"], f)] for f in firsts), variant
    V, T, cols, cell = S.shared_corners()
    r = reference(V, T, cols, cell, 2, 0)
    assert r["members"][0] == [0, 1, 2] and not r["fallback"][0] and r["took"][0] == 3
    assert sorted(np.isin(T, [0, 1, 2]).sum(axis=1).tolist()) == [0, 1, 1, 1, 2, 3]


@pytest.mark.parametrize("groups", [65535, 65537])
def test_large_groups(groups):
    V, T, cols, cell, (hub, big, mates) = S.large_groups(groups)
    s = M.simplify(V, T, cols, cell, 2, 0)
    assert s.groups == groups and len(s.vertex_index) == 3 + 1 + S.HUB_CORNERS
    sizes = np.bincount(s.rep, minlength=len(V))
    assert sizes[s.rep[big[0]]] == S.BIG_MEMBERS == 2 * S.TILE + 100 and np.all(s.rep[big] == s.rep[big[0]]) and s.vertex_map[big[0]] >= 0
    assert sizes[s.rep[hub]] == 1 + S.HUB_MATES and np.all(s.rep[mates] == s.rep[hub]) and s.vertex_map[hub] >= 0
    inc_start, _ = M.corner_lists(len(V), T)
    assert inc_start[hub + 1] - inc_start[hub] == S.HUB_CORNERS
    assert not np.array_equal(np.sort(big), np.arange(len(big)) + big.min())                # the members' indices are scattered
    # the reference's own lane-by-lane loops agree with the model on the two groups (the rest are groups of one vertex)
    for placement in (1, 2):
        want = M.simplify(V, T, cols, cell, placement, 0)
        r = reference(V, T, cols, cell, placement, 0, only={int(s.rep[hub]), int(s.rep[big[0]])})
        for v in (hub, big[0]):
            o = want.vertex_map[v]
            assert np.array_equal(W.bits(r["vertices"][o]), W.bits(want.vertices[o])) and np.array_equal(W.bits(r["colors"][o]), W.bits(want.colors[o]))
    assert groups % 64 != 0                                                                  # full waves and a partial one


def test_long_runs():
    V, T, cols, cell, where = S.long_runs()
    nt = len(T)
    s = {fl: M.simplify(V, T, cols, cell, 0, fl) for fl in (0, 1, 2)}
    assert s[0].groups == 26 and s[0].rep[26] == 25 and all(n > 2 * S.TILE for n in S.RUNS)
    assert [where[i][2] for i in range(3)] == list(S.RUNS) and where["deg"][2] == S.DEGENERATE_RUN and where["zero"][2] == S.ZERO_LO_RUN
    assert all(x.degenerate == S.DEGENERATE_RUN for x in s.values())
    for i, n in enumerate(S.RUNS):
        first, last, _ = where[i]
        assert 900 < first < last < nt - 200                                               # inside the array, not at its ends
        same = np.flatnonzero(np.all(np.sort(T, axis=1) == np.sort(S.RUN_SETS[i]), axis=1))
        assert len(same) == n and same[0] == first and same[-1] == last
        windings = [tuple(t) for t in T[same].tolist()]
        assert windings.count(windings[0]) == 1 and windings.count(windings[-1]) == 1       # the first and the last copy are recognisable
        assert first in s[0].triangle_index and not np.any(np.isin(same[1:], s[0].triangle_index))
        assert np.all(np.isin(same, s[1].triangle_index))
        assert (first in s[2].triangle_index) == (n % 2 == 1) and not np.any(np.isin(same[1:], s[2].triangle_index))
        o = np.searchsorted(s[0].triangle_index, first)
        assert tuple(s[0].triangles[3 * o:3 * o + 3]) == tuple(s[0].vertex_map[list(S.RUN_SETS[i])])   # its own winding: (a, b, c)
    zero = np.flatnonzero(np.all(np.sort(T, axis=1) == (0, 6, 10), axis=1))
    assert len(zero) == S.ZERO_LO_RUN and zero[0] in s[0].triangle_index and not np.any(np.isin(zero, s[2].triangle_index))   # an even run after the degenerate records
    for name, sets in S.FAMILY.items():
        for t in sets:
            same = np.flatnonzero(np.all(np.sort(T, axis=1) == np.sort(t), axis=1))
            assert len(same) == 2 and same[1] - same[0] == 9 and same[0] in s[0].triangle_index and same[1] not in s[0].triangle_index
            assert not np.any(np.isin(same, s[2].triangle_index))
        axis = {"lo": 0, "mid": 1, "hi": 2}[name]
        assert len({tuple(np.delete(np.sort(t), axis)) for t in sets}) == 1 and len({int(np.sort(t)[axis]) for t in sets}) == 3   # differ in that one only


@pytest.mark.parametrize("groups", S.BYTE_EDGES)
def test_byte_edges(groups):
    V, T, cols, cell = S.byte_edge(groups)
    s = M.simplify(V, T, cols, cell, 0, 0)
    nb = {2: 1, 3: 1, 255: 1, 256: 1, 257: 2, 65535: 2, 65536: 2, 65537: 3}[groups]
    assert s.groups == groups and M.index_bytes(groups) == nb and s.passes == W.passes(V, cell) + 3 * nb
    assert M.simplify(V, T, cols, cell, 0, 1).passes == W.passes(V, cell)
    if groups == 2:
        assert len(s.vertex_index) == 0 and len(s.triangle_index) == 0 and s.degenerate == len(T) and np.all(s.vertex_map == -1)
        return
    assert np.array_equal(s.rep[:groups], np.arange(groups))                              # vertex = group number
    live = T[~W.degenerate(T)]
    assert live.max() == groups - 1 and s.duplicates >= 2 * len(s.triangle_index) > 0        # every set is there three times or more
    top = groups - 1
    if top > 255:
        assert np.any(live >> (8 * (nb - 1)))                                           # a group number in the top byte
    if groups in (255, 256, 65535, 65536):                                                # pairs of sets that differ only in the top byte
        sets = np.unique(np.sort(live, axis=1), axis=0)
        shift = 8 * (nb - 1)
        low = sets & ((1 << shift) - 1) if shift else sets * 0
        for column in range(3):
            others = np.delete(sets, column, axis=1)
            found = False
            for a in range(len(sets)):
                twin = np.flatnonzero(np.all(others == others[a], axis=1) & (low[:, column] == low[a, column]) & (sets[:, column] != sets[a, column]))
                found = found or len(twin) > 0
            assert found, column


@pytest.mark.parametrize("nt", S.TRIANGLE_COUNTS)
def test_triangle_counts_do_not_follow_the_vertex_count(nt):
    V, T, cols, cell = S.many_triangles(nt)
    s = M.simplify(V, T, cols, cell, 2, 0)
    assert len(V) == 12 and len(T) == nt and 3 < s.groups < 12 and s.duplicates > nt // 4 and s.degenerate > nt // 4 and len(s.triangle_index) > 20


def _sorted_position(V, cell):
    """The place of every vertex's group in the order of the lattice key (z above y above x): the lane of k_ts_place is its % 256."""
    k = W.cells(V, cell)
    key = (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]
    return np.searchsorted(np.unique(key), key)


@pytest.mark.parametrize("kept", list(S.SHEET_TILES))
def test_tiled_sheets_fall_back_everywhere(kept):
    V, T, cols, cell = S.tiled_sheets(kept)
    s = M.simplify(V, T, cols, cell, 2, 0)
    assert s.groups == len(s.vertex_index) == s.fallbacks == kept
    assert np.array_equal(W.bits(s.vertices), W.bits(M.simplify(V, T, cols, cell, 1, 0).vertices))
    c = M.simplify(V, T, cols, cell, 2, 2)
    assert len(c.vertex_index) == 0 and c.fallbacks == 0                                  # sheet on sheet: nothing is kept, nothing is counted
    assert reference(V, T, cols, cell, 2, 2, "fallbacks_over_all_groups")["fallbacks"] == kept   # though every quadric would fall back


@pytest.mark.parametrize("pattern", list(S.LANE_PATTERNS))
def test_one_fallback_per_wave_sits_in_its_lane(pattern):
    V, T, cols, cell = S.one_per_wave(pattern)
    r = reference(V, T, cols, cell, 2, 0)
    want = S.LANE_PATTERNS[pattern]
    assert r["fallbacks"] == len(want) == M.simplify(V, T, cols, cell, 2, 0).fallbacks
    position = _sorted_position(V, cell)
    assert sorted(position[r["vertex_index"][r["fallback"]]].tolist()) == list(want)
    assert len(r["vertex_index"]) == r["groups"] == 256 + 2 * len(want)                   # one full block and a partial wave
    assert sorted(position[r["vertex_index"]].tolist()) == list(range(r["groups"]))


def test_census_is_exact():
    V, T, cols, cell, at = S.census()
    r = reference(V, T, cols, cell, 2, 0)
    s = M.simplify(V, T, cols, cell, 2, 0)
    U = S.U
    sizes = {n: [len(r["members"][int(r["rep"][v])]) for v in m] for n, m in at.items()}
    assert sizes == {"zero_area": [1, 1, 1], "low_face": [4] * 4, "high_face": [4] * 4, "cut_exact": [2, 2], "cut_above": [2, 2], "l0_small": [2, 2],
                     "unkept": [2, 2, 1]}
    fell = sorted(r["vertex_index"][r["fallback"]].tolist())
    assert fell == sorted(at["zero_area"].tolist() + [int(at["high_face"].min())]) and s.fallbacks == len(S.CENSUS_FALLBACKS) == 4
    row = lambda name: s.vertices[s.vertex_map[at[name][0]]].astype(f64) / U           # noqa: E731
    before = lambda name: np.array(r["before"][int(r["rep"][at[name][0]])]) / U        # noqa: E731
    took = lambda name: r["took"][int(r["rep"][at[name][0]])]                          # noqa: E731
    assert before("low_face").tolist() == [40.0, 2.0, 2.0] == row("low_face").tolist() and took("low_face") == 3      # ON the lower face: inside
    assert before("high_face").tolist() == [84.0, 2.0, 2.0] and took("high_face") == 3                                # ON the upper face: outside
    assert row("high_face").tolist() == [82.125, 1.875, 2.0]                                                          # the centroid
    assert took("zero_area") == 0 and row("zero_area").tolist() == [1.0, 1.0, 1.0]
    # the eigenvalues of the cut groups, exactly
    inc_start, inc = M.corner_lists(len(V), T)
    for name, diag in (("cut_exact", [2.0 ** 62, 0.0, float(S.CUT)]), ("cut_above", [2.0 ** 62, 0.0, float(S.CUT + 1)]),
                       ("l0_small", [0.0, 2.0 ** 62, float(S.CUT + 1)])):
        total = [0.0] * 9
        c = _mean([V[m] for m in at[name]], None)
        for m in at[name]:
            own = [0.0] * 9
            for e in inc[inc_start[m]:inc_start[m + 1]]:
                own = [a + b for a, b in zip(own, _triangle_terms(V[T[e // 3]], c, None))]
            total = [a + b for a, b in zip(total, own)]
        assert [total[0], total[3], total[5]] == diag and total[1] == total[2] == total[4] == 0.0, name
    assert float(S.CUT) == 1e-3 * 2.0 ** 62 and float(S.CUT + 1) == np.nextafter(f64(S.CUT), np.inf)    # the cut itself, and one ulp above it
    assert took("cut_exact") == 1 and row("cut_exact").tolist() == [121.0, 1.0, 2.0]                    # equal is not greater: z stays
    assert took("cut_above") == 2 and row("cut_above").tolist() == [161.0, 1.0, 1.0]
    assert took("l0_small") == 2 and row("l0_small").tolist() == [201.0, 1.0, 1.0]
    assert np.all(s.vertex_map[at["unkept"][:2]] == -1)
    inc = reference(V, T, cols, cell, 2, 0, "fallbacks_over_all_groups")["fallbacks"]
    assert inc == s.fallbacks + 2                                                          # the unkept pair and the lone vertex of its triangle


@pytest.mark.parametrize("name", list(S.SCALES))
def test_scaled_meshes_take_the_branches_of_the_unscaled_one(name):
    V, T, cols, cell = S.scaled_corner(name)
    V0, T0 = S.corner()
    r, r0 = reference(V, T, cols, cell, 2, 0), reference(V0, T0, None, 0.75, 2, 0)
    assert r["fallbacks"] == r0["fallbacks"] == 0
    ranks = lambda x: sorted(x["took"].values())                                           # noqa: E731
    assert ranks(r0).count(3) == 8 and set(ranks(r0)) == {1, 2, 3}
    if name != "subnormal":
        assert ranks(r) == ranks(r0) and np.array_equal(r["vertices"].astype(f64), r0["vertices"].astype(f64) * 2.0 ** S.SCALES[name])
    else:
        assert np.all(np.abs(V) < np.finfo(f32).tiny) and np.all(np.abs(r["vertices"]) < np.finfo(f32).tiny) and ranks(r).count(3) >= 8
        assert len(r["vertex_index"]) == len(r0["vertex_index"])
    assert np.all(np.isfinite(r["vertices"])) and (np.abs(V).max() > 2.0 ** 120 if name == "huge" else np.abs(V).max() < 2.0 ** -98)


# ---- the header against the model ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_simplify_stress") / "mesh_simplify_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cpp", "mesh_simplify_host.cpp"), "-o", exe])
    return exe


def _host(exe, tmp_path, V, T, cols, cell, placement, flags):
    src, dst = str(tmp_path / "simplify.in"), str(tmp_path / "simplify.out")
    with open(src, "wb") as f:
        f.write(struct.pack("<5q2f", len(V), len(T), flags, placement, int(cols is not None), cell, 0.0) + W.bits(V).tobytes()
                + np.ascontiguousarray(T, i32).tobytes() + (b"" if cols is None else np.ascontiguousarray(cols, f32).tobytes()))
    p = subprocess.run([exe, "simplify", src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "mesh simplify ok" in p.stdout, (p.returncode, p.stderr)
    return np.fromfile(dst, i64)


@pytest.mark.parametrize("name", list(CASES))
def test_header_matches_model_bit_for_bit(host_exe, tmp_path, name):
    from tests.test_mesh_simplify_host import _check
    V, T, cols, cell = case(name)
    for placement, flags in CASES[name][1]:
        _check(_host(host_exe, tmp_path, V, T, cols, cell, placement, flags), M.simplify(V, T, cols, cell, placement, flags), len(V), (name, placement, flags))
