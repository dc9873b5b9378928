"""Voxels.Redistance on the GPU (sdfk_volume_redistance, csrc/lib_redistance.hip) against the numpy model of the contract
(tests/redistance_model.py), bit for bit -- uint32 views, signed zeros included -- and, where the model is too slow (128^3,
256^3), against the g++ full-sweep host solver built from the same csrc/redistance.h (tests/cpp/redistance_host.cpp), which
tests/test_redistance_host.py pins to the model.  The block-active schedule must be the full Jacobi iteration exactly: the
sweep count and the number of tile-sweeps are compared with the model's too."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import redistance_model as M

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _vox(values, mn, mx, colors=None):
    from sdfkit_amd import Voxels
    return Voxels(np.array(values, f32), colors, mn, mx)


def _check(values, mn, mx, iso=0.0, band=INF, tiles=True):
    """GPU == model: values, sweeps, front and clamped counts, and the tile-sweeps of the block-active schedule."""
    h = M.cell_sizes(mn, mx, values.shape)
    st = {}
    got = _vox(values, mn, mx).Redistance(iso, band, stats=st).Values
    want, wst = M.redistance(values, h, iso, band)
    print(values.shape, "iso", iso, "band", band, "gpu", st, "model", wst)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[:4].T)], want[tuple(bad[:4].T)])
    assert st["sweeps"] == wst["sweeps"] and st["front"] == wst["front"] and st["clamped"] == wst["clamped"]
    if tiles:
        assert st["tile_sweeps"] == wst["tile_sweeps"]
    return got, st


def _two_spheres(shape, mn, mx):
    x, y, z = M.centres(mn, mx, shape)
    a = np.sqrt((x + 0.4) ** 2 + y * y + z * z) - 0.7
    b = np.sqrt((x - 0.5) ** 2 + (y - 0.2) ** 2 + (z + 0.1) ** 2) - 0.55
    return np.minimum(a, b)


@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_spheres_equal_model_bitwise(gpu, n, kind):
    v, h, _ = M.sphere_inputs(n, kind)
    _check(v, [-1.5] * 3, [1.5] * 3)


@pytest.mark.parametrize("seed", range(4))
def test_random_volumes_equal_model_bitwise(gpu, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (17, 17, 17)).astype(f32)
    mx = [1.0, 1.0, 1.0] if seed % 2 == 0 else [float(x) for x in rng.uniform(0.5, 3.0, 3)]
    _check(v, [0.0, 0.0, 0.0], mx)


def test_non_cubic_anisotropic_not_multiples_of_the_tile(gpu):
    shape, mn, mx = (40, 24, 56), [-1.5, -1.0, -1.2], [1.5, 1.1, 1.3]
    v = (_two_spheres(shape, mn, mx) * 2.5).astype(f32)   # |grad| = 2.5, a crease where the spheres meet
    _check(v, mn, mx)
    _check(v[:37, :19, :51], mn, mx)   # 37 x 19 x 51: ragged tiles along every axis (and other cell sizes)


def test_iso_value(gpu):
    v, h, _ = M.sphere_inputs(32, "b")
    _check(v, [-1.5] * 3, [1.5] * 3, iso=0.3)
    _check(v, [-1.5] * 3, [1.5] * 3, iso=-0.45)


def test_values_equal_to_iso_are_inside_with_negative_zero(gpu):
    v = np.ones((12, 9, 10), f32)
    v[3:7, 2:6, 4:8] = 0.0   # == iso: inside, T0 = 0 on its faces
    v[5, 4, 5] = -1.0
    got, _ = _check(v, [0, 0, 0], [1.2, 0.9, 1.0])
    assert np.signbit(got[3, 2, 4]) and got[3, 2, 4] == 0.0


def test_band_equals_clamp_of_unbanded(gpu):
    shape, mn, mx = (40, 24, 56), [-1.5, -1.0, -1.2], [1.5, 1.1, 1.3]
    v = (_two_spheres(shape, mn, mx) * 2.5).astype(f32)
    band = f32(3.0) * M.cell_sizes(mn, mx, shape)[0]
    full = _vox(v, mn, mx).Redistance().Values
    banded, st = _check(v, mn, mx, band=float(band))
    clamp = np.where(np.abs(full) < band, full, np.copysign(band, full)).astype(f32)
    assert np.array_equal(_bits(banded), _bits(clamp))
    assert st["clamped"] == int((np.abs(full) > band).sum()) > 0


def test_front_in_one_corner_tile_of_96_cubed(gpu):
    """The active set has to travel from one corner tile across 12^3 - 1 idle ones."""
    n, mn, mx = 96, [0.0] * 3, [9.6] * 3
    x, y, z = M.centres(mn, mx, (n, n, n))
    v = (np.sqrt((x - 0.33) ** 2 + (y - 0.31) ** 2 + (z - 0.36) ** 2) ** 2 - 0.25 ** 2).astype(f32)
    assert np.all(np.argwhere(v <= 0) < 8)
    _, st = _check(v, mn, mx)
    assert st["tile_sweeps"] < st["sweeps"] * 12 ** 3 // 4   # (what the active set saves)


def test_no_front(gpu):
    v = np.full((9, 20, 8), 0.5, f32)
    v[2, 3, 4] = 0.25
    got, st = _check(v, [0, 0, 0], [1, 2, 1])
    assert np.all(got == INF) and st["sweeps"] == 0 and st["front"] == 0
    got, st = _check(-v, [0, 0, 0], [1, 2, 1], band=0.75)
    assert np.all(got == f32(-0.75)) and st["clamped"] == v.size


def test_single_inside_voxel(gpu):
    v = np.ones((11, 11, 11), f32)
    v[5, 5, 5] = -1.0
    got, st = _check(v, [0, 0, 0], [1.1, 2.2, 3.3])
    assert st["front"] == 7 and got[5, 5, 5] < 0 and (got > 0).sum() == v.size - 1


def test_refusals_leave_dst_untouched(gpu):
    from sdfkit_amd import Voxels
    from sdfkit_amd import _native as N
    from sdfkit_amd._native import SdfKitNativeError
    lib = N.lib()
    good = np.random.default_rng(1).uniform(-1, 1, (10, 9, 8)).astype(f32)
    marker = np.full(good.shape, 7.0, f32)
    dst = Voxels(marker.copy(), None, [0, 0, 0], [1, 1, 1])
    hd = dst._sync_to_device()

    def refused(src_vox, iso, band, hdst=hd):
        r = lib.sdfk_volume_redistance(src_vox._sync_to_device(), hdst, C.c_float(iso), C.c_float(band), None)
        assert r == 1 and b"sdfk_volume_redistance" in lib.sdfk_last_error(), (r, lib.sdfk_last_error())   # SDFK_ERR_INVALID
        out = np.zeros(good.shape, f32)
        N.check(lib.sdfk_volume_download(hd, out.ctypes.data, None))
        assert np.array_equal(out, marker)
        return lib.sdfk_last_error().decode()

    for bad_value in (np.nan, np.inf, -np.inf):
        v = good.copy()
        v[9, 8, 7] = bad_value
        assert "NaN or infinite" in refused(Voxels(v, None, [0, 0, 0], [1, 1, 1]), 0.0, INF)
    src = Voxels(good, None, [0, 0, 0], [1, 1, 1])
    refused(src, np.nan, INF)
    refused(src, INF, INF)
    refused(src, 0.0, np.nan)
    refused(src, 0.0, -1.0)
    assert "shape or box" in refused(Voxels(good[:9], None, [0, 0, 0], [1, 1, 1]), 0.0, INF)
    assert "shape or box" in refused(Voxels(good, None, [0, 0, 0], [1, 1, 2]), 0.0, INF)
    with pytest.raises(SdfKitNativeError):
        src.Redistance(maxDistance=-2.0)
    with pytest.raises(SdfKitNativeError):
        src.Redistance(isoValue=np.nan)
    # the accepted call through the same handles works afterwards
    assert lib.sdfk_volume_redistance(src._sync_to_device(), hd, C.c_float(0.0), C.c_float(INF), None) == 0
    want, _ = M.redistance(good, M.cell_sizes([0, 0, 0], [1, 1, 1], good.shape))
    out = np.zeros(good.shape, f32)
    N.check(lib.sdfk_volume_download(hd, out.ctypes.data, None))
    assert np.array_equal(_bits(out), _bits(want))


def test_input_unchanged_colours_copied_versions(gpu):
    from sdfkit_amd import Sdfs, Voxels
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, (13, 10, 21)).astype(f32)
    col = rng.uniform(0, 1, (13, 10, 21, 3)).astype(f32)
    src = Voxels(v.copy(), col.copy(), [0, 0, 0], [1, 1, 2])
    v0 = src._version
    out = src.Redistance()
    assert src._version == v0 and out._version > 0
    assert (out.NX, out.NY, out.NZ) == (13, 10, 21) and np.array_equal(out.Min, src.Min) and np.array_equal(out.Max, src.Max)
    assert np.array_equal(_bits(out.Colors), _bits(col))
    assert np.array_equal(_bits(src.Values), _bits(v)) and np.array_equal(_bits(src.Colors), _bits(col))
    want, _ = M.redistance(v, M.cell_sizes([0, 0, 0], [1, 1, 2], v.shape))
    assert np.array_equal(_bits(out.Values), _bits(want))
    # a device-resident source (sampled, never downloaded) is left as it was, too
    dev = Voxels.SampleSdf(Sdfs.Sphere(0.8), [-1, -1, -1], [1, 1, 1], 20, 20, 20)
    v1 = dev._version
    red = dev.Redistance(maxDistance=0.3)
    assert dev._version == v1
    before = dev.Values.copy()
    want, _ = M.redistance(before, M.cell_sizes([-1] * 3, [1] * 3, before.shape), 0.0, 0.3)
    assert np.array_equal(_bits(red.Values), _bits(want))
    # an Sdf that reads the result binds the new volume
    assert np.isfinite(red.ToSdf().Sample(np.zeros((1, 3), f32))).all()


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return M.build_host_solver(tmp_path_factory.mktemp("redistance"))


@pytest.mark.parametrize("n,kind", [(128, "c"), (256, "b")])
def test_large_volumes_equal_host_solver_bitwise(gpu, host_exe, tmp_path, n, kind):
    v, h, _ = M.sphere_inputs(n, kind)
    if n == 128:   # something less symmetric than a sphere: a twisted, repeated field with creases
        x, y, z = M.centres([-1.5] * 3, [1.5] * 3, (n, n, n))
        v = np.maximum(v.astype(np.float64), 0.35 - np.abs(np.sin(4 * x) * np.cos(3 * y) + np.sin(5 * z) * 0.5)).astype(f32)
    st = {}
    got = _vox(v, [-1.5] * 3, [1.5] * 3).Redistance(stats=st).Values
    want, wst = M.host_solve(host_exe, v, h, 0.0, INF, tmp_path)
    print(n, "gpu", st, "host", wst)
    assert np.array_equal(_bits(got), _bits(want))
    assert st["sweeps"] == wst["sweeps"] and st["front"] == wst["front"]
    assert st["tile_sweeps"] < st["sweeps"] * (n // 8) ** 3


def test_banded_mesh_volume_to_full_field(gpu):
    """The loop the feature was built for: Sdf -> Mesh -> banded Voxels -> Redistance -> full field."""
    from sdfkit_amd import RayMarcher, Sdfs
    n, mn, mx = 128, [-1.5] * 3, [1.5] * 3
    dx = float(M.cell_sizes(mn, mx, (n, n, n))[0])
    mesh = Sdfs.Sphere(1.0).ToMesh(mn, mx, n, n, n)
    banded = mesh.ToVoxels(mn, mx, n, n, n, maxDistance=4 * dx)
    red = banded.Redistance()
    # (i) the result has the input's sign at every voxel, so marching cubes finds the same sign-changing edges (one vertex
    # each) and the same cell configurations (the triangles of a cell depend on its corner signs only)
    m0, m1 = banded.ToMesh(), red.ToMesh()
    assert len(m1.Vertices) == len(m0.Vertices) > 0 and len(m1.Triangles) == len(m0.Triangles) > 0
    b, r = banded.Values.copy(), red.Values.copy()
    assert np.array_equal(r > 0, b > 0)
    # (ii) far field: the first-order error recorded for the model at this size (tests/golden/redistance_accuracy.json) plus the
    # mesh's own chordal error, measured here as the worst deviation of the banded volume (an exact distance to the mesh) from
    # the sphere's distance inside the band
    with open(os.path.join(ROOT, "tests", "golden", "redistance_accuracy.json")) as f:
        acc = json.load(f)
    x, y, z = M.centres(mn, mx, (n, n, n))
    ana = np.sqrt(x * x + y * y + z * z) - 1.0
    err = np.abs(r.astype(np.float64) - ana) / dx
    far = np.abs(b) >= f32(4 * dx)
    chord = float((np.abs(b.astype(np.float64) - ana) / dx)[~far].max())
    bound = acc["sphere"]["128"]["a"]["max"] + chord
    print("loop 128^3: far-field max error %.4f voxels (mean %.4f); bound %.4f = recorded %.4f + chordal %.4f; the banded far field was "
          "wrong by up to %.1f voxels" % (err[far].max(), err[far].mean(), bound, acc["sphere"]["128"]["a"]["max"], chord,
                                          (np.abs(b.astype(np.float64) - ana) / dx)[far].max()))
    assert far.sum() > n ** 3 // 2 and err[far].max() <= bound
    # (iii) the ray marcher sees the sphere where tests/test_raymarch.py expects the analytic one
    w, h = 50, 30
    img = RayMarcher(w, h, red.ToSdf()).RenderDepth()
    print("centre depth", img[w // 2, h // 2])
    assert abs(img[w // 2, h // 2] - 4.0) <= 1.0e-2
