"""Voxels.Redistance on the GPU (sdfk_volume_redistance, csrc/lib_redistance.hip) on the stress cases of
tests/redistance_cases.py, bit for bit against the numpy model (tests/redistance_model.py): uint32 views of the values, sweeps,
front, clamped and tile_sweeps.  tests/test_redistance_cases.py asserts on the CPU what each case is for and pins the g++ host
solver to the model on all of them, so a mismatch here points at the device's arithmetic, layout or schedule.

New against tests/test_gpu_redistance.py: idle tiles that are swept again (no earlier input does that), the edges of the
32-sweep batches, volumes thinner than a tile, denormal / huge / mixed magnitudes, the edges of the band, and the sentences of
the contract that never ran on the device: in place, cached sign bits dropped, colours zeroed, slabs, and the refusal of cell
sizes that are not finite and > 0."""
import ctypes as C

import numpy as np
import pytest

from tests import redistance_cases as RC
from tests import redistance_model as M

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_bits(got, want, what=""):
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (what, len(bad), bad[:4], np.asarray(got)[tuple(bad[:4].T)], np.asarray(want)[tuple(bad[:4].T)])


def _check(c):
    """GPU == model on one case: values and all four stats."""
    from sdfkit_amd import Voxels
    st = {}
    got = Voxels(c.values.copy(), None, c.mn, c.mx).Redistance(c.iso, c.band, stats=st).Values
    want, wst = RC.model(c)
    print(c.name, c.values.shape, "gpu", st, "model", wst)
    _same_bits(got, want, c.name)
    assert st == wst, (c.name, st, wst)


def _ids(c):
    return c.name


# ---- 2. idle tiles that are swept again ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RC.reactivation_cases() + RC.reactivation_cases(banded=True), ids=_ids)
def test_idle_tiles_swept_again(gpu, c):
    _check(c)


# ---- 3. the edges of the 32-sweep batches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", range(3))
def test_fixed_point_at_the_batch_edges(gpu, axis):
    for n in RC.BATCH_N:
        _check(RC.line(n, axis))


# ---- 4. thin and ragged shapes ---------------------------------------------------------------------------------------------------
def test_thin_and_ragged_shapes(gpu):
    for c in RC.thin_cases():
        _check(c)


# ---- 5. extremes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RC.extreme_cases(), ids=_ids)
def test_extreme_magnitudes(gpu, c):
    _check(c)


# ---- 6. the edges of the band ----------------------------------------------------------------------------------------------------
def test_band_edges(gpu):
    for c in RC.band_cases():
        _check(c)


# ---- 7. the contract through the C ABI -------------------------------------------------------------------------------------------
class _Vol:
    """A volume handle of the C ABI (a slab when z0 / nz_global are given)."""

    def __init__(self, shape, mn, mx, colors=False, z0=0, nz_global=None):
        from sdfkit_amd import _native as N
        N.init()
        self.N, self.lib, self.shape, self.colors = N, N.lib(), tuple(shape), colors
        self.h = C.c_void_p()
        nx, ny, nz = shape
        N.check(self.lib.sdfk_volume_create_slab(nx, ny, nz if nz_global is None else nz_global, N.f3(np.asarray(mn, f32)),
                                                 N.f3(np.asarray(mx, f32)), z0, nz, 1 if colors else 0, C.byref(self.h)))

    def upload(self, values, colors=None):
        values = np.ascontiguousarray(values, f32)
        colors = None if colors is None else np.ascontiguousarray(colors, f32)
        self.N.check(self.lib.sdfk_volume_upload(self.h, values.ctypes.data, None if colors is None else colors.ctypes.data))
        return self

    def download(self):
        v = np.zeros(self.shape, f32)
        c = np.full(self.shape + (3,), -1.0, f32)
        self.N.check(self.lib.sdfk_volume_download(self.h, v.ctypes.data, c.ctypes.data))
        return v, c

    def redistance(self, dst, iso=0.0, band=INF):
        st = (C.c_int64 * 4)()
        r = self.lib.sdfk_volume_redistance(self.h, dst.h, C.c_float(iso), C.c_float(band), st)
        return r, dict(sweeps=int(st[0]), tile_sweeps=int(st[1]), front=int(st[2]), clamped=int(st[3]))

    def free(self):
        if self.h:
            self.lib.sdfk_volume_free(self.h)
            self.h = None


def _random_case(shape, seed, colors=True):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, shape).astype(f32), (rng.uniform(0, 1, tuple(shape) + (3,)).astype(f32) if colors else None)


@pytest.mark.parametrize("colors", [False, True])
def test_in_place(gpu, colors):
    shape, mn, mx = (13, 10, 21), [0, 0, 0], [1, 1, 2]
    v, col = _random_case(shape, 11, colors)
    vol = _Vol(shape, mn, mx, colors).upload(v, col)
    r, st = vol.redistance(vol, 0.1, 0.03)
    assert r == 0, vol.lib.sdfk_last_error()
    want, wst = M.redistance(v, M.cell_sizes(mn, mx, shape), 0.1, 0.03)
    got, gcol = vol.download()
    _same_bits(got, want)
    assert st == wst and 0 < wst["clamped"] < v.size
    if colors:
        assert np.array_equal(_bits(gcol), _bits(col))
    else:
        assert not gcol.any()
    # the wake-up case in place: the solve reads src only before it writes dst
    c = RC.reactivation_cases()[1]
    vol2 = _Vol(c.values.shape, c.mn, c.mx).upload(c.values)
    r, st = vol2.redistance(vol2)
    assert r == 0
    _same_bits(vol2.download()[0], RC.model(c)[0])
    assert st == RC.model(c)[1]
    vol.free(), vol2.free()


def _sampled_sphere(n=20):
    from sdfkit_amd import Sdfs, Voxels
    mn, mx = [-1.0] * 3, [1.0] * 3
    vox = Voxels.SampleSdf(Sdfs.Sphere(0.8), mn, mx, n, n, n)   # device resident: the sampler cached the sign bits about 0
    return vox, mn, mx


def test_in_place_drops_cached_sign_bits(gpu):
    from oracle import oracle as O
    from sdfkit_amd.api import Mesh
    from sdfkit_amd import _native as N
    from tests.test_gpu_parity import assert_mesh_equal
    vox, mn, mx = _sampled_sphere()
    lib, h = N.lib(), vox._h
    before = np.zeros((vox.NX, vox.NY, vox.NZ), f32)
    col = np.zeros(before.shape + (3,), f32)
    N.check(lib.sdfk_volume_download(h, before.ctypes.data, col.ctypes.data))
    N.check(lib.sdfk_volume_redistance(h, h, C.c_float(0.3), C.c_float(INF), None))
    want, _ = M.redistance(before, M.cell_sizes(mn, mx, before.shape), 0.3)
    assert ((want > 0) != (before > 0)).sum() > 100   # the sign pattern about 0 is another now
    m = C.c_void_p()
    N.check(lib.sdfk_march(h, C.c_float(0.0), 1, C.byref(m)))
    assert_mesh_equal(Mesh._from_handle(m), O.march(want, col, mn, mx, 0.0))
    after = np.zeros(before.shape, f32)
    N.check(lib.sdfk_volume_download(h, after.ctypes.data, None))
    _same_bits(after, want)


def test_separate_dst_meshed_before_drops_its_sign_bits(gpu):
    from oracle import oracle as O
    from sdfkit_amd.api import Mesh
    from sdfkit_amd import _native as N
    from tests.test_gpu_parity import assert_mesh_equal
    src, mn, mx = _sampled_sphere()
    dst, _, _ = _sampled_sphere()
    lib = N.lib()
    shape = (src.NX, src.NY, src.NZ)
    before, col = np.zeros(shape, f32), np.zeros(shape + (3,), f32)
    N.check(lib.sdfk_volume_download(src._h, before.ctypes.data, col.ctypes.data))
    m0 = C.c_void_p()
    N.check(lib.sdfk_march(dst._h, C.c_float(0.0), 1, C.byref(m0)))   # dst has been meshed at 0: whatever that cached is about the old values
    old = Mesh._from_handle(m0)
    assert_mesh_equal(old, O.march(before, col, mn, mx, 0.0))
    N.check(lib.sdfk_volume_redistance(src._h, dst._h, C.c_float(0.3), C.c_float(INF), None))
    want, _ = M.redistance(before, M.cell_sizes(mn, mx, shape), 0.3)
    m1 = C.c_void_p()
    N.check(lib.sdfk_march(dst._h, C.c_float(0.0), 1, C.byref(m1)))
    new = Mesh._from_handle(m1)
    assert_mesh_equal(new, O.march(want, col, mn, mx, 0.0))
    assert len(new.Vertices) != len(old.Vertices)
    # src still meshes as before
    m2 = C.c_void_p()
    N.check(lib.sdfk_march(src._h, C.c_float(0.0), 1, C.byref(m2)))
    assert_mesh_equal(Mesh._from_handle(m2), O.march(before, col, mn, mx, 0.0))


def test_colours_of_dst_zeroed_when_src_has_none(gpu):
    shape, mn, mx = (9, 10, 11), [0, 0, 0], [1, 1, 1]
    v, col = _random_case(shape, 12)
    src = _Vol(shape, mn, mx, colors=False).upload(v)
    dst = _Vol(shape, mn, mx, colors=True).upload(np.full(shape, 7.0, f32), col)
    r, st = src.redistance(dst)
    assert r == 0
    got, gcol = dst.download()
    want, wst = M.redistance(v, M.cell_sizes(mn, mx, shape))
    _same_bits(got, want)
    assert st == wst and np.array_equal(_bits(gcol), np.zeros(gcol.shape, np.uint32))
    # and copied when both have them
    src2 = _Vol(shape, mn, mx, colors=True).upload(v, col)
    dst.upload(np.full(shape, 7.0, f32), np.zeros_like(col))
    assert src2.redistance(dst)[0] == 0
    got, gcol = dst.download()
    _same_bits(got, want)
    assert np.array_equal(_bits(gcol), _bits(col))
    src.free(), src2.free(), dst.free()


def test_slab_is_solved_on_its_own_planes(gpu):
    nx, ny, nzg, z0, n = 13, 10, 40, 13, 11
    mn, mx = [0.0, -1.0, 0.5], [1.3, 1.0, 4.5]
    v, _ = _random_case((nx, ny, nzg), 13, colors=False)
    v[:, :, z0 + 4:] = np.abs(v[:, :, z0 + 4:]) + f32(0.125)   # somewhere to travel inside the slab; another front above it
    v[:, :, z0 + n + 2] *= -1
    planes = np.ascontiguousarray(v[:, :, z0:z0 + n])
    h = M.cell_sizes(mn, mx, (nx, ny, nzg))   # h_z = (max - min) / nz_global
    want, wst = M.redistance(planes, h)
    whole, _ = M.redistance(v, h)
    assert np.any(_bits(whole[:, :, z0:z0 + n]) != _bits(want)) and wst["sweeps"] >= 5   # (the planes alone: not a window of the whole)
    src = _Vol((nx, ny, n), mn, mx, z0=z0, nz_global=nzg).upload(planes)
    dst = _Vol((nx, ny, n), mn, mx, z0=z0, nz_global=nzg).upload(np.full(planes.shape, 7.0, f32))
    r, st = src.redistance(dst)
    assert r == 0, src.lib.sdfk_last_error()
    _same_bits(dst.download()[0], want)
    assert st == wst
    # a dst slab with another z0 is refused and left as it was
    other = _Vol((nx, ny, n), mn, mx, z0=z0 + 1, nz_global=nzg).upload(np.full(planes.shape, 7.0, f32))
    r, _ = src.redistance(other)
    assert r == 1 and b"shape or box" in src.lib.sdfk_last_error()
    assert np.all(other.download()[0] == f32(7.0))
    src.free(), dst.free(), other.free()


# ---- 8. / 9. refusals ------------------------------------------------------------------------------------------------------------
def test_cell_sizes_not_finite_and_positive_are_refused(gpu):
    """(A box of this kind is never run through the solve: with a negative cell size the model has no fixed point.)"""
    shape = (9, 10, 11)
    good, _ = _random_case(shape, 14, colors=False)
    marker = np.full(shape, 7.0, f32)
    for mn, mx in (([0, 0, 0], [1, -1, 1]), ([0, 0, 0], [-1, 1, 1]), ([0, 0, 2], [1, 1, 1]),     # max < min
                   ([0, 0, 0], [1, 0, 1]), ([0.5, 0, 0], [0.5, 1, 1]),                          # max == min
                   ([0, 0, 0], [np.nan, 1, 1]), ([0, np.nan, 0], [1, 1, 1]),                   # NaN
                   ([0, 0, 0], [1, 1, np.inf]), ([-np.inf, 0, 0], [1, 1, 1]), ([-3e38, 0, 0], [3e38, 1, 1])):   # infinite bound / size
        with np.errstate(all="ignore"):
            h = M.cell_sizes(mn, mx, shape)
        with pytest.raises(ValueError):
            M.redistance(good, h)
        src = _Vol(shape, mn, mx).upload(good)
        dst = _Vol(shape, mn, mx).upload(marker)
        for d in (dst, src):   # separate and in place
            r, _ = src.redistance(d)
            msg = src.lib.sdfk_last_error()
            assert r == 1 and b"sdfk_volume_redistance" in msg and b"cell sizes" in msg, (mn, mx, r, msg)   # SDFK_ERR_INVALID
        assert np.array_equal(_bits(dst.download()[0]), _bits(marker)) and np.array_equal(_bits(src.download()[0]), _bits(good))
        src.free(), dst.free()
    # A handle's box is fixed when it is created (the C ABI has no call that changes it), so the handles refused for their box
    # can only be freed.  The handles that "work afterwards, once they are given a proper volume" are a pair with a proper box,
    # refused for a NaN value first and then given finite values.
    src = _Vol(shape, [0, 0, 0], [1, 1, 1])
    dst = _Vol(shape, [0, 0, 0], [1, 1, 1]).upload(marker)
    bad = good.copy()
    bad[4, 5, 6] = np.nan
    src.upload(bad)
    assert src.redistance(dst)[0] == 1 and np.array_equal(_bits(dst.download()[0]), _bits(marker))
    src.upload(good)
    r, st = src.redistance(dst)
    assert r == 0
    want, wst = M.redistance(good, M.cell_sizes([0, 0, 0], [1, 1, 1], shape))
    _same_bits(dst.download()[0], want)
    assert st == wst
    src.free(), dst.free()


def test_python_layer_raises_for_a_flat_box(gpu):
    from sdfkit_amd import Voxels
    from sdfkit_amd._native import SdfKitNativeError
    good, _ = _random_case((9, 10, 11), 15, colors=False)
    with pytest.raises(SdfKitNativeError, match="cell sizes"):
        Voxels(good, None, [0, 0, 0], [1, 0, 1]).Redistance()
    with pytest.raises(SdfKitNativeError, match="cell sizes"):
        Voxels(good, None, [0, 0, 0], [1, -2, 1]).Redistance()
