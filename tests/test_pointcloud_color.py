"""CPU checks of per-point colours in the point-cloud pipeline: the numpy model (tests/pointcloud_color_model.py) on cases derivable
by hand, the shared arithmetic of the kernels (sdfkit_amd/csrc/points_color.h) built with g++ against the model bit for bit, and
the six new C-ABI entry points: exported, and refusing to run without a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from sdfkit_amd import _native as N
from tests import pointcloud_color_model as CM
from tests import pointcloud_model as PC
from tests import points_filter_model as FM
from tests import points_knn_model as KM

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["sdfk_points_blend_colors", "sdfk_points_blend_colors_device", "sdfk_points_to_volume_colors",
                "sdfk_points_to_volume_colors_device", "sdfk_points_voxel_downsample_colors", "sdfk_points_voxel_downsample_colors_device"]


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def _lattice(n=5):
    g = np.arange(n, dtype=f32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)


# ---- the model on hand-made cases ----
def test_k1_is_the_nearest_points_colour_and_nothing_found_is_zero():
    P = _lattice()
    col = np.random.default_rng(1).standard_normal((len(P), 3)).astype(f32)
    col[7] = [-0.0, np.inf, np.nan]                                    # nothing is clamped or checked
    Q = (P + f32(0.2)).astype(f32)
    out, found = CM.sample_colors(P, col, Q, 1)
    assert (found == 1).all() and np.array_equal(_bits(out), _bits(col))
    out, found = CM.sample_colors(P, col, [[50, 50, 50], [np.nan, 0, 0], [0, np.inf, 0]], 4, 1.0)
    assert (found == 0).all() and np.array_equal(_bits(out), np.zeros((3, 3), np.uint32))    # +0, bit for bit


def test_equal_distances_take_the_first_neighbour_and_weights_fall_to_zero_at_the_cutoff():
    P = _lattice(2)                                                    # the corners of a unit cube
    col = np.arange(24, dtype=f32).reshape(8, 3)
    Q = np.array([[0.5, 0.5, 0.5]], f32)
    out, found = CM.sample_colors(P, col, Q, 8)                        # every d2 equal to h2: W == 0
    assert found[0] == 8 and np.array_equal(out[0], col[0])
    # k = 2 of two points: the farther one is the cut-off and has weight 0, so the nearer one's colour comes back exactly
    out, _ = CM.sample_colors([[0, 0, 0], [1, 0, 0]], [[0.3, 0.6, 0.9], [5, 5, 5]], [[0.25, 0, 0]], 2)
    assert np.array_equal(_bits(out[0]), _bits(np.array([0.3, 0.6, 0.9], f32)))
    # a query on top of a point and its duplicate: h2 == 0, the lower index's colour
    out, found = CM.sample_colors([[1, 1, 1], [1, 1, 1], [3, 3, 3]], [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 1, 1]], 2)
    assert found[0] == 2 and np.array_equal(out[0], np.array([1, 0, 0], f32))
    # fewer than k within a finite max_distance: the cut-off is the radius bound, and the weights are (1 - d2 / bound)^2
    out, found = CM.sample_colors([[0, 0, 0], [1, 0, 0], [9, 0, 0]], [[1, 0, 0], [0, 1, 0], [7, 7, 7]], [[0.5, 0, 0]], 3, 2.0)
    assert found[0] == 2 and np.array_equal(out[0], np.array([0.5, 0.5, 0], f32))


def test_a_constant_colour_comes_back_bit_for_bit():
    """Every point has the colour c.  w c / w is not exact in binary64 for every c, but S_c / W differs from c by a few units of
    2^-53 relative (k + 1 roundings), far inside the half-ulp of the final rounding to float32 (2^-25), so every voxel with a
    neighbour gets c bit for bit -- for any finite normal float32 c, dyadic or not; the model confirms it, W == 0 voxels included
    (they take the first neighbour's colour)."""
    i = np.arange(300, dtype=np.float64) + 0.5
    phi, th = np.arccos(1 - 2 * i / 300), np.pi * (1 + 5 ** 0.5) * i
    P = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1).astype(f32)
    c = np.array([0.25, 0.75, 0.1], f32)
    for k, md in ((1, np.inf), (8, 0.4), (16, np.inf)):
        _, _, col, found = CM.to_volume(P, P, np.tile(c, (len(P), 1)), (-1.5,) * 3, (1.5,) * 3, (9, 8, 7), k, md)
        assert (found > 0).any() and (np.isinf(md) or (found == 0).any())
        assert (_bits(col[found > 0]) == _bits(c)).all() and (_bits(col[found == 0]) == 0).all()


def test_model_volume_values_are_the_colourless_models():
    rs = np.random.default_rng(3)
    P = rs.random((200, 3), dtype=f32)
    Nn = rs.standard_normal((200, 3)).astype(f32)
    Nn[::9] = 0
    v, known, col, found = CM.to_volume(P, Nn, rs.random((200, 3), dtype=f32), (0, 0, 0), (1, 1, 1), (6, 5, 7), 4, 0.2)
    want, wknown = PC.to_volume(P, Nn, (0, 0, 0), (1, 1, 1), (6, 5, 7), 4, 0.2)
    assert np.array_equal(_bits(v), _bits(want)) and np.array_equal(known, wknown)
    assert ((found > 0) & ~known).any() and (col[(found > 0) & ~known] != 0).any()   # a colour without a value


def test_group_means_by_hand():
    col = np.array([[1, 2, -0.0], [3, 4, 5], [5, 6, 7], [-0.0, -0.0, -0.0]], f32)
    out = CM.group_means(col, [0, 1, 0, 2], 3)
    assert np.array_equal(_bits(out), _bits(np.array([[3, 4, 3.5], [3, 4, 5], [0.0, 0.0, 0.0]], f32)))   # a lone -0.0: +0.0


# ---- the kernels' arithmetic, built for the host ----
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("points_color_host")
    exe = str(d / "points_color_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "points_color_host.cpp"), "-o", exe])

    def run(mode, data):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(data, f32).tofile(fin)
        p = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and f"points_color_host {mode} ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
        return np.fromfile(fout, f32).reshape(-1, 3)
    return run


def _host_blend(host, P, col, Q, k, md):
    """The host header on the model's knn rows -> (host colours, model colours, found, d2, h2 == 0 mask)."""
    idx, _, found = KM.knn(P, Q, k, md)
    with np.errstate(all="ignore"):
        d2 = PC._d2(P, Q, idx)
    want = CM.blend_rows(col, d2, found, k, md, idx)
    slots = np.zeros((len(Q), 64, 4), f32)
    slots[:, :k, :3] = col[np.maximum(idx, 0)]
    slots[:, :k, 3] = np.where(np.arange(k)[None, :] < found[:, None], d2, 0)
    rows = np.concatenate([found[:, None].astype(f32), slots.reshape(len(Q), -1)], axis=1)
    got = host("blend", np.concatenate([np.array([len(Q), k, md], f32), rows.reshape(-1)]))
    return got, want, found, d2


BLEND_CASES = {
    # name: (k, max_distance, what must occur)
    "lattice_ties": (9, np.inf, "ties"),
    "k1": (1, np.inf, "full"),
    "on_a_point": (3, np.inf, "h2_zero"),
    "all_equal_d2": (8, np.inf, "w_zero"),
    "short_finite": (16, 0.9, "short"),
    "short_inf": (64, np.inf, "short"),
    "nothing": (8, 0.05, "none"),
}


@pytest.mark.parametrize("name", sorted(BLEND_CASES))
def test_host_blend_equals_the_model(host, name):
    k, md, must = BLEND_CASES[name]
    rs = np.random.default_rng(sorted(BLEND_CASES).index(name))
    P = _lattice()
    Q = (rs.random((300, 3), dtype=f32) * f32(4)).astype(f32)
    if name == "on_a_point":
        P = np.concatenate([P, P, P])                                  # every point three times: the three nearest of a point are at 0
        Q = P[rs.integers(0, len(P), 300)]
    elif name == "all_equal_d2":
        Q = (_lattice(4) + f32(0.5)).astype(f32)                       # cell centres: eight corners at the same d2
    elif name == "short_inf":
        P = P[:40]
    elif name == "nothing":
        Q = (Q + f32(0.5) + rs.random((300, 3), dtype=f32) * f32(1e-3)).astype(f32) + f32(10)
    elif name == "lattice_ties":
        Q[:100] = np.round(Q[:100] * 2) / 2                            # on points, edges and centres: mass ties of d2
    col = FM.mixed_magnitudes(rs, len(P)) - f32(0.25)                  # sums whose order shows
    col[::11, 1] = -0.0
    got, want, found, d2 = _host_blend(host, P, col, Q, k, md)
    assert np.array_equal(_bits(got), _bits(want))
    last = d2[np.arange(len(Q)), np.maximum(found - 1, 0)]
    occurred = {
        "ties": ((found == k) & (d2[:, max(k - 2, 0)] == last) & (d2[:, 0] < last)).any(),    # a tie across the cut-off
        "full": (found == k).all(),
        "h2_zero": ((found == k) & (last == 0)).all(),
        "w_zero": ((found == k) & (d2[:, 0] == last) & (last > 0)).all(),
        "short": ((found > 0) & (found < k)).all(),
        "none": (found == 0).all(),
    }[must]
    assert occurred, (name, np.bincount(found, minlength=k + 1))
    if must in ("h2_zero", "w_zero") or k == 1:
        first = col[KM.knn(P, Q, 1)[0][:, 0]]
        assert np.array_equal(_bits(got), _bits(first))                # the first neighbour's colour, bit for bit
    if must == "none":
        assert (_bits(got) == 0).all()


def test_host_group_mean_equals_the_model(host):
    rs = np.random.default_rng(5)
    counts = [1, 32, 33, 100, 1, 64, 65, 2]
    group = np.repeat(np.arange(len(counts)), counts)
    order = rs.permutation(len(group))                                 # members scattered over the insertion order
    group = group[order]
    relabel = np.full(len(counts), -1)                                 # groups numbered in the order of their lowest member
    for g in group:
        if relabel[g] < 0:
            relabel[g] = relabel.max() + 1
    group = relabel[group]
    sizes = np.bincount(group)
    col = FM.mixed_magnitudes(rs, len(group)) - f32(0.125)
    lone = np.flatnonzero(sizes[group] == 1)
    col[lone[0]] = [-0.0, 1.5, -0.0]                                   # a lone member's -0.0 comes back as +0.0
    col[np.flatnonzero(sizes[group] == 33), 2] = -0.0                  # a whole channel of -0.0: +0.0 as well (the sums start at +0.0)
    want = CM.group_means(col, group, len(counts))
    data = [np.array([len(counts)], f32)]
    for g in range(len(counts)):
        members = np.flatnonzero(group == g)                           # ascending index
        data += [np.array([len(members)], f32), col[members].reshape(-1)]
    got = host("mean", np.concatenate(data))
    assert np.array_equal(_bits(got), _bits(want))
    assert sorted(sizes) == sorted(counts)
    g0 = group[lone[0]]
    assert np.array_equal(_bits(got[g0]), _bits(np.array([0.0, 1.5, 0.0], f32)))
    assert (_bits(got[sizes == 33][:, 2]) == 0).all()


def test_model_downsample_keeps_the_colourless_outputs():
    rs = np.random.default_rng(8)
    P = rs.random((500, 3), dtype=f32)
    col = rs.random((500, 3), dtype=f32)
    pts, cnt, group, out = CM.voxel_downsample(P, col, 0.25)
    p0, c0, g0 = FM.voxel_downsample(P, 0.25)
    assert np.array_equal(_bits(pts), _bits(p0)) and np.array_equal(cnt, c0) and np.array_equal(group, g0) and out.shape == pts.shape
    pts, cnt, group, out = CM.voxel_downsample(P, col, 1e-4)           # below the spacing: the colours in order
    assert (cnt == 1).all() and np.array_equal(_bits(out), _bits(col))
    # the same call averages normals, or coordinates: the centroid is the mean of the points themselves
    pts, _, _, out = CM.voxel_downsample(P, P, 0.25)
    assert np.array_equal(_bits(out), _bits(pts))


# ---- recorded accuracy ----
def test_recorded_colour_accuracy_is_the_models():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "pointcloud_color_accuracy.json")) as f:
        rec = json.load(f)
    assert rec == CM.accuracy_figures()
    assert rec["vertex_color_error_max"] < 0.25 * 3 * (3.0 / rec["grid"])   # a condition: below the colour's change over the band


# ---- the C ABI ----
def test_color_entry_points_exported():
    L = N.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in N.SIGNATURES, name


def test_color_entry_points_refuse_without_device():
    """No device (or sdfk_init not called): every new entry point returns SDFK_ERR_NO_DEVICE, in a fresh process."""
    p = subprocess.run([sys.executable, "-c", "from tests.test_pointcloud_color import _refusals; _refusals(); print('refusals ok')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "refusals ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def _refusals():
    L = N.lib()
    a = np.zeros((3, 3), f32)
    A = C.c_void_p(a.ctypes.data)
    calls = {
        "sdfk_points_blend_colors": lambda: L.sdfk_points_blend_colors(None, A, A, 3, 8, np.inf, A, None),
        "sdfk_points_blend_colors_device": lambda: L.sdfk_points_blend_colors_device(None, A, A, 3, 8, np.inf, A, None),
        "sdfk_points_to_volume_colors": lambda: L.sdfk_points_to_volume_colors(None, A, A, None, 8, np.inf, None),
        "sdfk_points_to_volume_colors_device": lambda: L.sdfk_points_to_volume_colors_device(None, A, A, None, 8, np.inf, None),
        "sdfk_points_voxel_downsample_colors": lambda: L.sdfk_points_voxel_downsample_colors(None, 1.0, None, A, A, None, None, A, None),
        "sdfk_points_voxel_downsample_colors_device": lambda: L.sdfk_points_voxel_downsample_colors_device(None, 1.0, None, A, A, None, None, A, None),
    }
    assert sorted(calls) == sorted(ENTRY_POINTS)
    for name, call in calls.items():
        assert call() == N.ERR_NO_DEVICE, name
