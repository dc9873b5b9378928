"""Properties of the numpy model of Voxels.Redistance (tests/redistance_model.py; contract: include/sdfkit_hip.h,
"Redistancing") and its measured first-order accuracy, pinned to tests/golden/redistance_accuracy.json
(tools/gen_redistance_accuracy.py).  The model is deterministic: recomputed figures must EQUAL the recorded ones.
Idempotence is not claimed (a second pass re-derives the front from the first pass' values)."""
import json
import os

import numpy as np
import pytest

from tests import redistance_model as M

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "redistance_accuracy.json")) as f:
        return json.load(f)


def _aniso_case(seed=3, shape=(21, 14, 18)):
    rng = np.random.default_rng(seed)
    mn, mx = [-1.0, -0.5, 0.0], [1.1, 0.9, 0.8]
    x, y, z = M.centres(mn, mx, shape)
    v = (np.sin(3 * x) * np.cos(4 * y) + z - 0.4 + rng.uniform(-0.05, 0.05, shape)).astype(f32)
    return v, M.cell_sizes(mn, mx, shape)


@pytest.mark.parametrize("iso", [0.0, 0.2])
def test_sign_is_the_inputs_and_front_voxels_keep_t0(iso):
    v, h = _aniso_case()
    assert len(set(h.tolist())) == 3   # DX != DY != DZ
    out, st = M.redistance(v, h, iso)
    outside, frozen, t0 = M.front(v, h, iso)
    assert np.array_equal(outside, v.astype(f64) - f64(f32(iso)) > 0)
    assert np.array_equal(~np.signbit(out), outside)           # the sign BIT: -0.0 is inside
    assert np.array_equal(_bits(np.abs(out)[frozen]), _bits(t0[frozen]))
    assert st["front"] == int(frozen.sum()) > 0 and st["clamped"] == 0 and np.all(np.isfinite(out))
    # every voxel off the front lies farther than some neighbour (the upwind solve is causal)
    P = np.pad(np.abs(out), 1, constant_values=np.inf)
    nmin = np.minimum.reduce([P[:-2, 1:-1, 1:-1], P[2:, 1:-1, 1:-1], P[1:-1, :-2, 1:-1], P[1:-1, 2:, 1:-1], P[1:-1, 1:-1, :-2], P[1:-1, 1:-1, 2:]])
    assert np.all(np.abs(out)[~frozen] >= nmin[~frozen])


def test_front_value_by_hand():
    """One crossing on x at a third of DX, one on z at half of DZ: the distance to the plane through both."""
    v = np.ones((3, 3, 3), f32)
    v[1, 1, 1] = -1.0
    v[0, 1, 1] = 2.0          # t_x = DX * 1 / (1 + 2) towards -x, DX * 1 / 2 towards +x: the least wins
    v[1, 0, 1] = v[1, 2, 1] = -1.0
    h = np.array([0.3, 0.5, 0.2], f32)
    _, frozen, t0 = M.front(v, h)
    tx, tz = f64(h[0]) * 1.0 / 3.0, f64(h[2]) * 1.0 / 2.0
    assert frozen[1, 1, 1] and t0[1, 1, 1] == f32(1.0 / np.sqrt(1.0 / (tx * tx) + 1.0 / (tz * tz)))
    assert t0[0, 1, 1] == f32(f64(h[0]) * 2.0 / 3.0)           # a single-axis front: the crossing itself


def test_update_by_hand():
    h = np.array([0.5, 0.5, 0.5])
    one = M.update(np.array([[1.0], [np.inf], [np.inf]]), h)
    assert one[0] == f32(1.5)
    two = M.update(np.array([[np.inf], [1.0], [1.0]]), h)      # sorted: y, z, then x unused
    assert two[0] == f32(1.0 + 0.5 / np.sqrt(2.0))
    three = M.update(np.array([[1.0], [1.0], [1.0]]), h)
    assert abs(float(three[0]) - (1.0 + 0.5 / np.sqrt(3.0))) < 1e-6
    far = M.update(np.array([[1.0], [1.6], [3.0]]), h)         # a_1 + h <= a_2: the first axis alone
    assert far[0] == f32(1.5)


def test_accuracy_equals_the_recorded_measurements(recorded):
    for n in (16, 32, 64):
        for kind in "abc":
            got, want = M.sphere_record(n, kind), recorded["sphere"][str(n)][kind]
            print(n, kind, got)
            assert got == want, (n, kind, got, want)
            if kind != "a":   # the point of the feature: closer to the true distance than it started
                assert got["max"] < got["input_max"] and got["mean"] < got["input_mean"]
            # the zero set stays where marching cubes places it on the input, to the recorded tolerance (exact only for single-axis fronts)
            assert got["edge_shift"] <= recorded["sphere"][str(n)][kind]["edge_shift"] < 0.5


def test_exact_sphere_changes_by_no_more_than_the_first_order_error(recorded):
    for n in (16, 32):
        v, h, d = M.sphere_inputs(n, "a")
        out, _ = M.redistance(v, h)
        moved = np.abs(out.astype(f64) - v.astype(f64)) / float(h[0])
        # |out - v| <= |out - d| + |d - v|: the recorded error plus the f32 rounding of the input
        assert moved.max() <= recorded["sphere"][str(n)]["a"]["max"] + 1e-5


@pytest.mark.parametrize("name", ["box", "two_spheres"])
def test_accuracy_against_the_marching_cubes_mesh_of_the_input(recorded, name):
    got = M.mesh_record(name)
    print(name, got)
    assert got == recorded["mesh"][name]
    assert got["max"] < got["input_max"] and got["mean"] < got["input_mean"]


def test_band_equals_clamp_of_unbanded_bitwise():
    v, h = _aniso_case(seed=4)
    full, fst = M.redistance(v, h)
    for vox in (0.0, 0.5, 2.0, 5.0):
        band = f32(vox) * h[1]
        banded, st = M.redistance(v, h, 0.0, band)
        clamp = np.where(np.abs(full) < band, full, np.copysign(band, full)).astype(f32)
        assert np.array_equal(_bits(banded), _bits(clamp)), vox
        assert st["clamped"] == int((np.abs(full) > band).sum()) and st["sweeps"] <= fst["sweeps"]
    v3, h3, _ = M.sphere_inputs(32, "c")
    full, fst = M.redistance(v3, h3)
    banded, st = M.redistance(v3, h3, 0.0, f32(3) * h3[0])
    assert np.array_equal(_bits(banded), _bits(np.where(np.abs(full) < f32(3) * h3[0], full, np.copysign(f32(3) * h3[0], full)).astype(f32)))
    assert st["sweeps"] < fst["sweeps"] // 2 and st["tile_sweeps"] < fst["tile_sweeps"]   # it stops expanding at the band


def test_no_front():
    v = np.full((5, 6, 7), 2.0, f32)
    out, st = M.redistance(v, [1, 1, 1])
    assert np.all(out == np.inf) and st == {"sweeps": 0, "tile_sweeps": 0, "front": 0, "clamped": 0}
    out, st = M.redistance(-v, [1, 1, 1], 0.0, 1.5)
    assert np.all(out == f32(-1.5)) and st["clamped"] == v.size
    out, _ = M.redistance(np.zeros((4, 4, 4), f32), [1, 1, 1], 0.0, 1.5)   # v == iso everywhere: all inside, no front
    assert np.all(out == f32(-1.5))


def test_single_inside_voxel():
    v = np.ones((9, 9, 9), f32)
    v[4, 4, 4] = -1.0
    h = np.array([0.1, 0.2, 0.4], f32)
    out, st = M.redistance(v, h)
    assert st["front"] == 7 and (out < 0).sum() == 1
    t = 1.0 / np.sqrt(sum(1.0 / (f64(x) * 0.5) ** 2 for x in h))
    assert out[4, 4, 4] == -f32(t) and out[3, 4, 4] == f32(f64(h[0]) * 0.5) and out[4, 4, 5] == f32(f64(h[2]) * 0.5)
    assert out[0, 4, 4] == f32(f64(out[1, 4, 4]) + f64(h[0]))   # one axis alone along the row


def test_values_equal_to_iso_are_inside_at_distance_zero():
    v = np.ones((8, 8, 8), f32)
    v[2:5, 2:5, 2:5] = 0.25
    out, st = M.redistance(v, [1, 1, 1], 0.25)
    inside = np.zeros(v.shape, bool)
    inside[2:5, 2:5, 2:5] = True
    assert np.array_equal(np.signbit(out), inside)
    assert out[2, 3, 3] == 0.0 and np.signbit(out[2, 3, 3])     # on the front: T0 = 0 -> -0.0
    assert out[3, 3, 3] == -f32(np.sqrt(3.0) / 3.0)              # the centre voxel: three axes at a = 0, h = 1 -> 1 / sqrt(3)
    assert out[1, 3, 3] == 1.0                                   # outside, the crossing at the inside voxel's centre


def test_refusals():
    good = np.ones((3, 3, 3), f32)
    for bad in (np.nan, np.inf):
        v = good.copy()
        v[1, 1, 1] = bad
        with pytest.raises(ValueError):
            M.redistance(v, [1, 1, 1])
    for iso, band in ((np.nan, np.inf), (np.inf, np.inf), (0.0, np.nan), (0.0, -1.0)):
        with pytest.raises(ValueError):
            M.redistance(good, [1, 1, 1], iso, band)
