"""Inputs that stress Voxels.Redistance (include/sdfkit_hip.h, "Redistancing") where the first GPU tests never went: tiles of the
block-active schedule that go idle and are swept again, the edges of the 32-sweep batches, volumes thinner than a tile, extreme
magnitudes and the edges of the band.  tests/test_redistance_cases.py asserts on the CPU what each case is for (so that a later
edit cannot hollow it out) and pins the g++ host solver to the model on every one; tests/test_gpu_redistance_stress.py compares
the device with the model on the same list.

A case is (name, values f32, min, max, iso, band); its cell sizes are redistance_model.cell_sizes(min, max, values.shape)."""
from collections import namedtuple

import numpy as np

from tests import redistance_model as M

f32 = np.float32
INF = float("inf")
Case = namedtuple("Case", "name values mn mx iso band")


def cell_sizes(c):
    return M.cell_sizes(c.mn, c.mx, c.values.shape)


def model(c, **kw):
    return M.redistance(c.values, cell_sizes(c), c.iso, c.band, **kw)


def _case(name, values, mx, iso=0.0, band=INF, mn=(0.0, 0.0, 0.0)):
    return Case(name, np.ascontiguousarray(values, f32), [float(x) for x in mn], [float(x) for x in mx], float(iso), float(band))


def _ones_with_inside(shape, inside):
    v = np.ones(shape, f32)
    for p in inside:
        v[p] = -1.0
    return v


# ---- 2. idle tiles that are swept again -----------------------------------------------------------------------------------------
# One-voxel insides in a volume of ones with strongly anisotropic cells: the wave along the coarse axes settles a tile within a
# few sweeps, the slow wave along the fine axis arrives many sweeps later with smaller values and wakes it.
# (name, shape, max corner, inside voxels, sweeps, idle gaps, band of the banded variant)
REACTIVATION_SPECS = [
    ("wake_16x64x1", (16, 64, 1), (16.0, 1.0, 1.0), [(12, 3, 0), (3, 59, 0)], 64, {3, 5, 19, 21, 35, 36}, 0.75),
    ("wake_17x41x9", (17, 41, 9), (17.0, 41.0 / 32.0, 4.5), [(13, 2, 4), (2, 38, 4), (8, 20, 8)], 57, {2, 3, 11}, 0.75),
    # h = (1 / 32, 1 / 2, 1 / 2).  Tile (0, 0, 0) is left alone in sweep 6 and CHANGES in sweep 7, the sweep that wakes it: a
    # sweep reads face neighbours only, so that change comes in at the tile's corner from the tile diagonally across, in the one
    # sweep in which no face neighbour changed.  (Found by a search over random sign patterns, reduced to the voxels it needs.)
    ("wake_at_once_16x24x1", (16, 24, 1), (0.5, 12.0, 0.5),
     [(1, 10, 0), (3, 5, 0), (3, 7, 0), (4, 1, 0), (4, 3, 0), (4, 12, 0), (4, 14, 0), (5, 6, 0), (6, 9, 0), (7, 5, 0), (10, 6, 0), (11, 1, 0),
      (11, 3, 0), (14, 6, 0), (14, 8, 0)], 20, {1}, 0.75),
]
# a band BETWEEN two values the solve reaches (the tests check that on the model) for the re-activation and thin cases
BETWEEN = {"wake_16x64x1": 0.4, "wake_17x41x9": 0.4, "wake_at_once_16x24x1": 0.4}


def reactivation_cases(banded=False):
    out = []
    for name, shape, mx, inside, _, _, band in REACTIVATION_SPECS:
        v = _ones_with_inside(shape, inside)
        out.append(_case(name + ("_banded" if banded else ""), v, mx, band=band if banded else INF))
    return out


# ---- 3. the edges of the 32-sweep batches ---------------------------------------------------------------------------------------
BATCH_N = (33, 34, 35, 65, 66, 67)   # sweeps = N - 1: the fixed point in the last sweep of a batch, the first and second of the next


def line(n, axis, band=INF):
    shape = [1, 1, 1]
    shape[axis] = n
    v = np.ones(shape, f32)
    v[(0, 0, 0)] = -1.0
    mx = [1.0, 1.0, 1.0]
    mx[axis] = float(n)   # unit cells
    return _case("line%d_axis%d%s" % (n, axis, "" if band == INF else "_band%g" % band), v, mx, band=band)


def batch_cases():
    return [line(n, a) for a in range(3) for n in BATCH_N]


# ---- 4. thin and ragged shapes --------------------------------------------------------------------------------------------------
THIN_SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 9, 1), (7, 8, 9), (8, 8, 8), (9, 1, 17), (1, 16, 16), (16, 1, 16), (16, 16, 1),
               (3, 3, 200)]


def _random(shape, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(f32)


def thin_cases(band=INF, tag=""):
    out = [_case("thin_%dx%dx%d%s" % (s + (tag,)), _random(s, 40 + i), (1.0, 2.0, 3.0), band=band) for i, s in enumerate(THIN_SHAPES)]
    for p in ((7, 7, 7), (8, 8, 8)):   # a front on both sides of a tile corner
        out.append(_case("corner_%d%s" % (p[0], tag), _ones_with_inside((16, 16, 16), [p]), (1.0, 2.0, 3.0), band=band))
    return out


# ---- 5. extremes ----------------------------------------------------------------------------------------------------------------
def _half_outside(seed=7):
    v = _random((9, 10, 11), seed)
    v[4:] = np.abs(v[4:]) + f32(0.125)   # the planes x >= 4 are outside: the solve has somewhere to travel
    return v


def extreme_cases():
    v = _half_outside()
    aniso = (9e-3, 10.0, 11e3)   # h = (1e-3, 1, 1e3), nearly
    sel = np.random.default_rng(8).uniform(size=v.shape) < 0.5
    small = np.copysign(np.maximum(np.abs(v), 0.25), v).astype(np.float64) * 1e-44   # (one to seven units of the last denormal place)
    mix = np.where(sel, small, v.astype(np.float64) * 3e38).astype(f32)
    big = f32(2.9e38)
    near = (big + v.astype(np.float64) * 2e37).astype(f32)   # values on both sides of an iso near 3e38
    return [
        _case("box_1e-37", v, (1e-37, 2e-37, 3e-37)),   # DX is an f32 denormal, DY and DZ just above; most results are denormals
        _case("box_1e30_1e-30_1", v, (1e30, 1e-30, 1.0)),
        _case("box_3e38", v, (3e38, 3e38, 3e38)),
        _case("values_3e38", v * f32(3e38), aniso),
        _case("values_1e-40", (v.astype(np.float64) * 1e-40).astype(f32), aniso),
        _case("values_1e-44_and_3e38", mix, aniso),
        _case("iso_2.9e38", near, aniso, iso=float(big)),
        _case("iso_-2.9e38", -near, aniso, iso=-float(big)),
    ]


# ---- 6. the edges of the band ---------------------------------------------------------------------------------------------------
BAND_LINE = {0.0: 40, 0.25: 40, 0.5: 38, 1.5: 37, 2.5: 36, 3.0: 36}   # band -> clamped voxels of the 40-voxel line


def band_cases():
    out = [line(40, 0, band=b) for b in BAND_LINE]
    for b, tag in ((0.0, "_band0"), (None, "_between")):
        for c in reactivation_cases():
            out.append(c._replace(name=c.name + tag, band=BETWEEN[c.name] if b is None else b))
        for c in thin_cases():
            out.append(c._replace(name=c.name + tag, band=THIN_BETWEEN if b is None else b))
    return out


THIN_BETWEEN = 0.05


def all_cases():
    return reactivation_cases() + reactivation_cases(banded=True) + batch_cases() + thin_cases() + extreme_cases() + band_cases()
