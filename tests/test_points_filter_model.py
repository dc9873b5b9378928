"""CPU checks of the KdTree's two filters: the numpy model (tests/points_filter_model.py) on hand-made cases and on the recorded
sphere-with-strays case, the shared arithmetic of the kernels (sdfkit_amd/csrc/points_filter.h) built with g++ against the model,
and the four new C-ABI entry points: exported, and refusing to run without a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from sdfkit_amd import _native as N
from tests import points_filter_model as FM

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["sdfk_points_voxel_downsample", "sdfk_points_voxel_downsample_device", "sdfk_points_outliers", "sdfk_points_outliers_device"]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def recorded_case():
    """2000 points on the unit sphere and 20 strays: -> (points (2020, 3) float32, the strays' indices)."""
    rng = np.random.default_rng(5)
    s = rng.standard_normal((2000, 3))
    s = (s / np.linalg.norm(s, axis=1, keepdims=True)).astype(f32)
    u = rng.uniform(-4, 4, (40, 3))
    u = u[np.abs(np.linalg.norm(u, axis=1) - 1.0) > 0.5][:20].astype(f32)
    assert len(u) == 20
    return np.concatenate([s, u]), np.arange(2000, 2020)


def slow_downsample(P, size, origin=(0, 0, 0)):
    """The contract in plain Python loops, voxel by voxel."""
    P = np.asarray(P, f32).reshape(-1, 3)
    o = np.asarray(origin, f32)
    vox = {}
    for i, p in enumerate(P):
        key = tuple(int(np.floor((f64(p[a]) - f64(o[a])) / f64(f32(size)))) for a in range(3))
        vox.setdefault(key, []).append(i)          # (dicts keep insertion order: voxels by their lowest member)
    pts, cnt, group = [], [], np.empty(len(P), np.int32)
    for g, members in enumerate(vox.values()):
        total = np.zeros(3, f64)
        for a in range(0, len(members), 32):
            chunk = np.zeros(3, f64)
            for i in members[a:a + 32]:
                chunk = chunk + P[i].astype(f64)
            total = total + chunk
        pts.append((total / f64(len(members))).astype(f32))
        cnt.append(len(members))
        group[members] = g
    return np.array(pts, f32).reshape(-1, 3), np.array(cnt, np.int32), group


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- the model on hand-made cases ----
def test_floor_not_truncation_for_negative_coordinates():
    P = np.array([[-0.5, 0, 0], [0.5, 0, 0], [-1.5, 0, 0], [-1.0, 0, 0]], f32)
    pts, cnt, group = FM.voxel_downsample(P, 1.0)
    assert list(group) == [0, 1, 2, 0] and list(cnt) == [2, 1, 1]      # -0.5 and -1.0 share voxel -1; 0.5 is voxel 0 (truncation: with -0.5)
    assert np.array_equal(pts[0], np.array([-0.75, 0, 0], f32))


def test_points_exactly_on_voxel_faces():
    below = np.nextafter(f32(1.0), f32(0.0))
    P = np.array([[1.0, 0, 0], [below, 0, 0], [1.5, 0, 0], [np.nextafter(f32(1.5), f32(0)), 0, 0]], f32)
    _, cnt, group = FM.voxel_downsample(P, 0.5)
    assert list(group) == [0, 1, 2, 0] and list(cnt) == [2, 1, 1]      # a face belongs to the voxel above it


def test_a_non_zero_origin_moves_the_lattice():
    P = np.array([[0.1, 0.1, 0.1], [0.9, 0.1, 0.1], [1.2, 0.1, 0.1]], f32)
    assert list(FM.voxel_downsample(P, 1.0)[2]) == [0, 0, 1]
    assert list(FM.voxel_downsample(P, 1.0, (0.5, 0, 0))[2]) == [0, 1, 1]
    assert same(FM.voxel_downsample(P, 1.0, (0.5, 0.25, -3)), slow_downsample(P, 1.0, (0.5, 0.25, -3)))


def test_negative_zero_shares_the_voxel_of_zero_and_comes_back_positive():
    P = np.array([[-0.0, 0.0, -0.0], [5, 5, 5], [0.0, -0.0, 0.25]], f32)
    pts, cnt, group = FM.voxel_downsample(P, 1.0)
    assert list(group) == [0, 1, 0] and list(cnt) == [2, 1]
    # a lone -0.0: the sum starts at +0.0, so the coordinate comes back as +0.0 (the contract's step 3)
    pts, _, _ = FM.voxel_downsample(P[:2], 1.0)
    assert list(bits(pts[0])) == [0, 0, 0] and np.array_equal(bits(pts[1]), bits(P[1]))


@pytest.mark.parametrize("members", [1, 31, 32, 33, 64, 65, 1000])
def test_chunked_centroid_of_a_full_voxel(members):
    rs = np.random.default_rng(members)
    P = FM.mixed_magnitudes(rs, members, 10.0)   # (the order of the additions shows in the last bits)
    others = np.array([[40, 40, 40], [70, 70, 70]], f32)
    Q = np.concatenate([others[:1], P[:members // 2], others[1:], P[members // 2:]])
    got, want = FM.voxel_downsample(Q, 16.0), slow_downsample(Q, 16.0)
    assert same(got, want) and sorted(got[1]) == sorted([1, 1, members])
    if members == 1000:   # the chunking is part of the contract: one sequential chain gives another binary64 sum
        chain = np.zeros(3, f64)
        for p in P:
            chain = chain + p.astype(f64)
        total, _ = FM.chunked_sums(P.astype(f64), np.zeros(members, np.int64), np.arange(members), 1)
        assert not np.array_equal(chain, total[0]) and np.array_equal(bits((total[0] / f64(members)).astype(f32)), bits(got[0][1]))


def test_size_below_the_spacing_is_the_identity():
    rs = np.random.default_rng(3)
    P = (rs.permutation(4000)[:900, None] * f32(0.01) + rs.random((900, 3)) * 0.001 + 0.01).astype(f32)   # (no -0.0)
    pts, cnt, group = FM.voxel_downsample(P, 0.002)
    assert np.array_equal(bits(pts), bits(P)) and (cnt == 1).all() and np.array_equal(group, np.arange(900))


def test_span_of_2_21_voxels_is_refused():
    ok = np.array([[0, 0, 0], [2 ** 21 - 1, 0, 0]], f32)
    assert list(FM.voxel_downsample(ok, 1.0)[2]) == [0, 1]
    for axis in range(3):
        bad = np.zeros((2, 3), f32)
        bad[1, axis] = 2 ** 21
        with pytest.raises(FM.Refused):
            FM.voxel_downsample(bad, 1.0)
    for size in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(FM.Refused):
            FM.voxel_downsample(ok, size)
    with pytest.raises(FM.Refused):
        FM.voxel_downsample(ok, 1.0, (np.inf, 0, 0))
    # far from the origin the voxel numbers are beyond every integer type; what counts is their difference
    far = np.array([[3e38, 0, 0], [3e38, 0, 0]], f32)
    assert list(FM.voxel_downsample(far, 1e-30)[1]) == [2]


def test_model_against_the_plain_loops_on_a_random_cloud():
    rs = np.random.default_rng(9)
    P = (rs.standard_normal((3000, 3)) * 2).astype(f32)
    for size, origin in ((0.5, (0, 0, 0)), (1.25, (0.3, -0.2, 7)), (100.0, (0, 0, 0))):
        assert same(FM.voxel_downsample(P, size, origin), slow_downsample(P, size, origin))


def test_merged_sphere_numbers():
    """The merged scan of the issue: the sphere and a copy moved by 0.001, voxels of 0.1."""
    P, _ = recorded_case()
    P = P[:2000]
    M = np.concatenate([P, (P + f32(0.001)).astype(f32)])
    pts, cnt, group = FM.voxel_downsample(M, 0.1)
    assert len(pts) == 1079 and cnt.max() == 16 and cnt.sum() == 4000


# ---- the recorded outlier case ----
@pytest.mark.parametrize("k", [4, 8, 16])
def test_recorded_case_keeps_the_surface_and_removes_the_strays(k):
    P, strays = recorded_case()
    mean = FM.row_means(P, k)
    for ratio in (1.0, 2.0, 3.0):
        mu, sigma, thr, c = FM.threshold(mean, ratio)
        keep = mean <= thr
        assert c == len(P) and keep[:2000].all() and not keep[strays].any(), (k, ratio)
    out = FM.outliers(P, k, 2.0)
    assert list(out["stats"][:3]) == [2000, 20, 0] and np.array_equal(out["index"], np.arange(2000))


def test_outlier_model_edge_cases():
    # duplicates: the dropped first entry is the point or its lower duplicate; the rest of the row holds a zero distance
    P = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 2, 0]], f32)
    assert list(FM.row_means(P, 3)) == [0.5, 0.5, 1.0, 2.0]
    # a finite max_distance isolates: found < 2 -> +inf, no part in the statistics, never kept
    mean = FM.row_means(P, 3, 1.5)
    assert list(mean) == [0.5, 0.5, 1.0, np.inf]
    out = FM.outliers(P, 3, 0.0, 1.5)
    assert list(out["stats"][:3]) == [2, 1, 1] and list(out["keep"]) == [1, 1, 0, 0] and np.isinf(out["mean_distance"][3])
    # c = 0
    out = FM.outliers(P[2:], 2, 1.0, 0.5)
    assert list(out["stats"]) == [0, 0, 2, 0, 0, 0] and not out["keep"].any()
    for bad in ((1, 1.0, np.inf), (65, 1.0, np.inf), (8, -1.0, np.inf), (8, np.nan, np.inf), (8, np.inf, np.inf), (8, 1e39, np.inf),
                (8, 1.0, -1.0), (8, 1.0, np.nan)):                       # (1e39 rounds to +inf in f32, the type of the argument)
        with pytest.raises(FM.Refused):
            FM.outliers(P, *bad)


def test_an_infinite_ratio_would_keep_nothing_where_sigma_is_zero():
    """Why +inf is refused: with every mean equal, sigma == 0 and thr = mu + inf * 0 is a NaN, under which no point is kept; every
    finite ratio keeps every point of such a cloud."""
    P = np.tile(np.array([[0.25, 0.5, 0.75]], f32), (40, 1))
    mean = FM.row_means(P, 8)
    with np.errstate(all="ignore"):
        mu, sigma, thr, c = FM.threshold(mean, np.inf)
    assert c == 40 and sigma == 0 and np.isnan(thr) and not (mean <= thr).any()
    for ratio in (0.0, 1.0, 3e38):
        out = FM.outliers(P, 8, ratio)
        assert list(out["stats"][:3]) == [40, 0, 0] and not np.isnan(out["thr"])


# ---- points_filter.h, built for the host ----
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("points_filter_host")
    exe = str(d / "points_filter_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "points_filter_host.cpp"), "-o", exe])

    def run(mode, data, dtype):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        data.tofile(fin)
        p = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and f"points_filter_host {mode} ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
        return np.fromfile(fout, dtype)
    return run


def _key_input(P, size, origin):
    return np.concatenate([np.array([size, *origin, len(P)], f32), np.asarray(P, f32).reshape(-1)])


def test_host_key_equals_the_model(host):
    rs = np.random.default_rng(31)
    clouds = [((rs.standard_normal((500, 3)) * 3).astype(f32), 0.25, (0, 0, 0)),
              ((rs.standard_normal((500, 3)) * 3).astype(f32), 0.3, (0.1, -7.5, 3)),
              (np.array([[-0.0, 0.0, -0.5], [0.0, -0.0, -1.0], [1.0, np.nextafter(f32(1), f32(0)), 0.5]], f32), 0.5, (0, 0, 0)),
              (np.array([[0, 0, 0], [2 ** 21 - 1, 5, 70000]], f32), 1.0, (0, 0, 0)),
              (np.array([[3e38, -3e38, 0], [3e38, -3e38, 1e-30]], f32), 1e-30, (0, 0, 0)),
              ((rs.random((300, 3)) * 1e-3).astype(f32), 1.0, (0, 0, 0))]
    for P, size, origin in clouds:
        out = host("key", _key_input(P, size, origin), np.int64)
        keys, _ = FM.voxel_keys(P, size, origin)
        assert out[0] == 0 and np.array_equal(out[2:].view(np.uint64), keys)
        assert out[1] == sum(1 << d for d in FM.passes(P, size, origin))
    assert host("key", _key_input(clouds[-1][0], 1.0, (0, 0, 0)), np.int64)[1] == 0          # one voxel: no pass at all
    assert bin(host("key", _key_input(clouds[3][0], 1.0, (0, 0, 0)), np.int64)[1]).count("1") >= 6


def test_host_range_refusal_equals_the_model(host):
    for axis in range(3):
        for span, status in ((2 ** 21 - 1, 0), (2 ** 21, 3), (2 ** 22, 3)):
            P = np.zeros((2, 3), f32)
            P[1, axis] = span
            assert host("key", _key_input(P, 1.0, (0, 0, 0)), np.int64)[0] == status
            if status:
                with pytest.raises(FM.Refused):
                    FM.voxel_keys(P, 1.0)
    P = np.array([[0, 0, 0], [1, 1, 1]], f32)
    for size, status in ((0.0, 1), (-1.0, 1), (np.inf, 1), (np.nan, 1), (1e-45, 3), (1.0, 0)):
        assert host("key", _key_input(P, size, (0, 0, 0)), np.int64)[0] == status
    for o in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
        assert host("key", _key_input(P, 1.0, o), np.int64)[0] == 2
    assert host("key", _key_input(np.array([[-3e38, 0, 0], [3e38, 0, 0]], f32), 1.0, (0, 0, 0)), np.int64)[0] == 3


def test_host_chunked_sum_equals_the_model(host):
    rs = np.random.default_rng(32)
    counts = [1, 2, 31, 32, 33, 63, 64, 65, 1000, 1024, 1025]
    voxels = [FM.mixed_magnitudes(rs, c, 10.0) for c in counts]
    voxels.append(np.array([[-0.0, -0.0, -0.0]], f32))
    flat = [np.array([len(voxels)], f32)]
    for v in voxels:
        flat += [np.array([len(v)], f32), v.reshape(-1)]
    out = host("sum", np.concatenate(flat), f32).reshape(-1, 3)
    for v, got in zip(voxels, out):
        want, cnt, _ = FM.voxel_downsample(v, 1e6, (-5e5, -5e5, -5e5))      # one voxel holds them all
        assert len(want) == 1 and cnt[0] == len(v) and np.array_equal(bits(got), bits(want[0]))


def test_host_threshold_and_keep_rule_equal_the_model(host):
    P, _ = recorded_case()
    rows = []
    want = []
    for k, ratio, maxd in ((4, 1.0, np.inf), (8, 2.0, np.inf), (16, 0.0, np.inf), (8, 2.5, 0.05), (2, 1.0, 1e-6)):
        mean = FM.row_means(P, k, maxd)
        part = mean < np.inf
        mu, sigma, thr, c = FM.threshold(mean, ratio)
        with np.errstate(all="ignore"):
            s = FM.PM.reduce_fixed(np.where(part, mean, 0.0))
            d = np.where(part, mean, mu) - mu
            sq = FM.PM.reduce_fixed(np.where(part, d * d, 0.0))
        for i in (0, 7, 1999, 2000, 2019, int(np.argmax(np.where(part, mean, -1))), int(np.argmin(mean))):
            iso = not part[i]
            # (a row's sum and count that give this mean: the mean itself over one neighbour)
            rows.append([s, sq, c, ratio, 0.0 if iso else mean[i], 1 if iso else 2])
            want.append([mu, sigma, thr, mean[i], float(part[i] and mean[i] <= thr)])
    rows.append([0.0, 0.0, 0, 1.0, 3.0, 4])
    want.append([0.0, 0.0, 0.0, 1.0, 0.0])               # c = 0: the threshold is 0.0
    rows.append([6.0, 0.0, 3, 2.0, 6.0, 4])
    want.append([2.0, 0.0, 2.0, 2.0, 1.0])               # sigma = 0: a mean equal to the threshold is kept
    data = np.concatenate([np.array([len(rows)], f64), np.array(rows, f64).reshape(-1)])
    out = host("thr", data, f64).reshape(-1, 5)
    assert np.array_equal(out.view(np.uint64), np.array(want, f64).view(np.uint64))
    assert (out[:, 4] == 1).any() and (out[:, 4] == 0).any() and np.isinf(out[:, 3]).any()


def test_host_ratio_refusal_equals_the_model(host):
    """ratio_is_valid: finite and not negative.  Both zeros, the least subnormal and FLT_MAX pass; NaN of either sign, a negative
    number and both infinities do not -- and the model refuses exactly those."""
    ratios = np.array([0.0, -0.0, 1e-45, 0.1, 2.0, 3e38, np.finfo(f32).max, np.inf, -np.inf, np.nan, -np.nan, -1e-45, -1.0], f32)
    want = [1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    assert list(host("ratio", ratios, np.int64)) == want
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], f32)
    for r, ok in zip(ratios, want):
        if ok:
            FM.outliers(P, 2, r)
        else:
            with pytest.raises(FM.Refused):
                FM.outliers(P, 2, r)


# ---- the C ABI ----
def test_filter_entry_points_exported():
    L = N.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in N.SIGNATURES, name


def test_filters_refuse_without_device():
    """No device (or sdfk_init not called): the four entry points return SDFK_ERR_NO_DEVICE, in a fresh process."""
    p = subprocess.run([sys.executable, "-c", "from tests.test_points_filter_model import _refusals; _refusals(); print('refusals ok')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "refusals ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def _refusals():
    L = N.lib()
    a = np.zeros((3, 3), f32)
    A = C.c_void_p(a.ctypes.data)
    m = C.c_int64()
    for name in ENTRY_POINTS[:2]:
        assert getattr(L, name)(None, 1.0, None, A, None, None, C.byref(m)) == N.ERR_NO_DEVICE, name
    for name in ENTRY_POINTS[2:]:
        assert getattr(L, name)(None, 8, 2.0, np.inf, A, None, None, None, C.byref(m), None) == N.ERR_NO_DEVICE, name
