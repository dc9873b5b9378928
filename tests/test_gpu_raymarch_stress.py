"""The ray marcher on the MI355X under the tables of tests/raymarch_cases.py: sdfk_raymarch (JIT kernel, csrc/sample_codegen.h) and
its two entry points (csrc/lib_volume.hip), whole images bit for bit -- NaN == NaN, finite values to the sign bit -- against the C
oracle (oracle/sdfk_oracle_ray.c) over the scene catalogue and against the numpy model (tests/mathops_model.py,
tests/voxel_sdf_model.py) over IR programs.  tests/test_raymarch_cases.py shows on the CPU that the references' images hold what
these comparisons need: sky and hits, backward marches, all-sky and all-NaN frames, NaN colours on sound depths.

  cameras and lenses, through RayMarcher's properties and through Sdf.ToImage; 0, 1, 2, 40 and 400 steps; image shapes around the
  256-lane block, 1 and 2 pixels wide or high, wider and higher than 65 536; depth and colour in one call; sdfk_raymarch_device into
  caller-owned buffers with guard pixels; refusals; a pinned destination;
  the ray kernel's constants: one module for forty radii, constants baked as literals, programs that keep all literals, special
  values as arguments;
  random compositions of the catalogue; the mathops scenes and a bound volume from a camera inside their bodies."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from sdfkit_amd import Matrix4x4, RayMarcher, SdfExprs, Voxels
from sdfkit_amd import _native as N
from sdfkit_amd.api import Sdf
from sdfkit_amd.expr import MathF, Vec4, trace, trace_bound
from tests import mathops_model as M
from tests import raymarch_cases as R
from tests import scenes as S
from tests import voxel_sdf_model as VM

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = f32(-7.0)


def _marcher(sdf, camera, lens=R.DEFAULT_LENS, size=R.SWEEP_SIZE, iterations=40):
    rm = RayMarcher(size[0], size[1], sdf)
    with np.errstate(all="ignore"):      # (`degenerate_up` is NaN on purpose)
        rm.ViewTransform = Matrix4x4.CreateLookAt(*(R.CAMERAS[camera] if isinstance(camera, str) else camera))
    rm.VerticalFieldOfViewDegrees, rm.NearPlaneDistance, rm.FarPlaneDistance = lens
    rm.DepthIterations = iterations
    return rm


def _images(rm):
    """(depth, rgb) through the two public calls of the mirror"""
    with np.errstate(all="ignore"):
        d, c = rm.RenderDepth(), rm.Render()
    assert (d.Width, d.Height) == (rm.width, rm.height) == (c.Width, c.Height)
    return d.Values, c.Values


def _check(got, want, what):
    (gd, gc), (wd, wc) = got, want
    assert R.same_image(gd, wd), f"{what}: depth differs in {int(np.sum(~((gd == wd) | (np.isnan(gd) & np.isnan(wd)))))} pixels"
    assert R.same_image(gc, wc), f"{what}: colour differs in {int(np.sum(~((gc == wc) | (np.isnan(gc) & np.isnan(wc)))))} floats"


def _args(rm):
    """the C ABI arguments of a marcher up to (and without) the two destinations"""
    with np.errstate(all="ignore"):
        pos, vpi = rm.camera()
    return [rm.sdf.program(), rm.width, rm.height, N.f3(pos), (C.c_float * 16)(*[float(x) for x in vpi.ravel()]),
            C.c_float(rm.NearPlaneDistance), C.c_float(rm.FarPlaneDistance), int(rm.DepthIterations)]


def _host(rm, want_depth=True, want_rgb=True):
    """ONE sdfk_raymarch call into fresh numpy arrays pre-filled with the guard value"""
    depth, rgb = np.full((rm.height, rm.width), GUARD, f32), np.full((rm.height, rm.width, 3), GUARD, f32)
    N.check(N.lib().sdfk_raymarch(*_args(rm), depth.ctypes.data if want_depth else None, rgb.ctypes.data if want_rgb else None))
    return depth, rgb


def _untouched(a):
    return bool((np.asarray(a) == GUARD).all())


def _jit():
    a, b, c = C.c_int64(), C.c_int64(), C.c_double()
    N.check(N.lib().sdfk_jit_stats(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value


def _raymarch_launches(call):
    """launches of the ray kernel the profiler records while `call` runs"""
    L = N.lib()
    N.check(L.sdfk_profile_reset())
    N.check(L.sdfk_profile_enable(1))
    try:
        call()
    finally:
        N.check(L.sdfk_profile_enable(0))
    return sum(v[1] for k, v in N.profile_snapshot().items() if "raymarch" in k)


# ---- cameras and lenses --------------------------------------------------------------------------------------------------------
ROWS = [(cam, R.DEFAULT_LENS) for cam in R.CAMERAS] + [(cam, lens) for cam in ("oblique", "inside") for lens in R.LENSES[1:]]


@pytest.mark.parametrize("name", R.SWEEP_SCENES)
def test_cameras_and_lenses(gpu, name):
    sdf = S.CATALOGUE[name]()[1]
    for cam, lens in ROWS:
        _check(_images(_marcher(sdf, cam, lens)), R.catalogue_render(name, cam, lens), (name, cam, lens))
    # SdfEx.ToImage with a view matrix and every keyword is RayMarcher.Render
    cam, lens = "inside", (45.0, 0.5, 250.0)
    img = sdf.ToImage(*R.SWEEP_SIZE, Matrix4x4.CreateLookAt(*R.CAMERAS[cam]), verticalFieldOfViewDegrees=lens[0],
                      nearPlaneDistance=lens[1], farPlaneDistance=lens[2], depthIterations=40)
    assert (img.Width, img.Height) == R.SWEEP_SIZE
    assert R.same_image(img.Values, _marcher(sdf, cam, lens).Render().Values) and R.same_image(img.Values, R.catalogue_render(name, cam, lens)[1])


@pytest.mark.parametrize("name", ["plane_w", "sdf_with_color", "union8"])
def test_far_plane_exactly_at_a_depth(gpu, name):
    """`depth > far` is strict: the far plane at the exact depth of the middle pixel (through the C ABI, where the far plane of the
    sky test is an argument of its own), and at the near start with no step at all (through the mirror's properties)"""
    sdf = S.CATALOGUE[name]()[1]
    pos, vpi, far, depth, rgb = R.far_at_a_hit(name)
    rm = _marcher(sdf, "default")
    mirror = rm.camera()
    assert np.array_equal(mirror[0], pos) and np.array_equal(mirror[1], vpi)
    rm.FarPlaneDistance = far
    a = _args(rm)
    a[3], a[4] = N.f3(pos), (C.c_float * 16)(*[float(x) for x in vpi.ravel()])      # (the matrix of the default lens)
    gd, gc = np.full(depth.shape, GUARD, f32), np.full(rgb.shape, GUARD, f32)
    N.check(N.lib().sdfk_raymarch(*a, gd.ctypes.data, gc.ctypes.data))
    _check((gd, gc), (depth, rgb), (name, far))
    lens = (60.0, 1.0, float(f32(1.0) - f32(0.1)))
    _check(_images(_marcher(sdf, "default", lens, iterations=0)), R.catalogue_render(name, "default", lens, iterations=0), (name, lens))


# ---- iterations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cam", [("union8", "up_z"), ("sphere_w", "default")])
def test_iterations(gpu, name, cam):
    sdf = S.CATALOGUE[name]()[1]
    for iterations in R.ITERATIONS:
        got = _images(_marcher(sdf, cam, iterations=iterations))
        want = R.catalogue_render(name, cam, iterations=iterations)
        _check(got, want, (name, cam, iterations))
        if iterations == 0:      # no step: the near start, and a zero diffuse (0.1 ambient where it is not sky)
            assert np.array_equal(got[0], np.full(got[0].shape, f32(1.0) - f32(0.1), f32))
            assert np.array_equal(got[1], np.full(got[1].shape, f32(0.0) + (f32(0.1) * f32(1.0) + f32(0.0)), f32))
    one = R.catalogue_render(name, cam, iterations=1)[0]
    assert not np.array_equal(one, R.catalogue_render(name, cam, iterations=0)[0]) and not np.array_equal(one, R.catalogue_render(name, cam, iterations=2)[0])


# ---- shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(gpu, shape):
    sdf = S.readme_repeat_xy()[1]
    got = _images(_marcher(sdf, "oblique", size=shape, iterations=25))
    _check(got, R.catalogue_render("readme_repeat_xy", "oblique", size=shape, iterations=25), shape)
    if min(shape) == 1:
        assert np.isnan(got[0]).all() and np.isnan(got[1]).all()


# ---- one call for both images ----------------------------------------------------------------------------------------------------
def test_depth_and_colour_in_one_call(gpu):
    for name, cam, lens, size in [("readme_repeat_xy", "oblique", R.DEFAULT_LENS, (86, 3)), ("union8", "inside", (60.0, 0.05, R.INF), (33, 21))]:
        rm = _marcher(S.CATALOGUE[name]()[1], cam, lens, size)
        both = _host(rm)
        depth_only, rgb_only = _host(rm, want_rgb=False), _host(rm, want_depth=False)
        _check(both, R.catalogue_render(name, cam, lens, size), (name, cam))
        assert R.same_image(depth_only[0], both[0]) and _untouched(depth_only[1])
        assert R.same_image(rgb_only[1], both[1]) and _untouched(rgb_only[0])


def test_neither_image_is_ok_and_does_nothing(gpu, tmp_path):
    # a program no other test builds, so that a launch would have to compile its ray kernel first
    sdf = Sdf(lambda p: Vec4.of((0, 0, 0), (MathF.Sqrt((p.x * p.x + p.y * p.y) + p.z * p.z) - 0.8125) + (p.z - p.z)), False)
    rm = _marcher(sdf, "default")
    L = N.lib()
    N.check(L.sdfk_set_cache_dir(str(tmp_path / "jit").encode()))
    try:
        before = _jit()
        assert _raymarch_launches(lambda: N.check(L.sdfk_raymarch(*_args(rm), None, None))) == 0
        assert _raymarch_launches(lambda: N.check(L.sdfk_raymarch_device(*_args(rm), None, None))) == 0
        assert _jit() == before, "a call that asks for no image compiled or loaded a kernel"
        assert _raymarch_launches(lambda: _host(rm)) == 1      # (the counter does see a launch)
        assert sum(_jit()) == sum(before) + 1
    finally:
        N.check(L.sdfk_set_cache_dir(None))


# ---- the device entry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(86, 3), (2, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_entry_equals_host_form(gpu, size):
    """sdfk_raymarch_device into caller-owned buffers, asynchronously on the bound stream.  Both buffers have the length of the
    colour image plus a guard pixel and are pre-filled with -7: whatever lies beyond the image asked for still reads -7 afterwards,
    and so does all of a buffer that was not asked for.  The device images are checked first, against the oracle; the host form
    of the same call comes last and has the same bits."""
    import torch
    rm = _marcher(S.readme_repeat_xy()[1], "oblique", size=size, iterations=25)
    n = size[0] * size[1]
    want = R.catalogue_render("readme_repeat_xy", "oblique", size=size, iterations=25)
    L = N.lib()
    N.bind_torch_stream()
    dev = torch.device("cuda:0")
    got = {}
    try:
        for want_depth, want_rgb in [(True, False), (False, True), (True, True), (False, False)]:
            dd = torch.full((3 * (n + 1),), float(GUARD), dtype=torch.float32, device=dev)
            cd = torch.full((3 * (n + 1),), float(GUARD), dtype=torch.float32, device=dev)
            N.check(L.sdfk_raymarch_device(*_args(rm), C.c_void_p(dd.data_ptr()) if want_depth else None,
                                           C.c_void_p(cd.data_ptr()) if want_rgb else None))
            torch.cuda.synchronize()
            d, c = dd.cpu().numpy(), cd.cpu().numpy()
            if want_depth:
                assert R.same_image(d[:n].reshape(want[0].shape), want[0]) and _untouched(d[n:]), (want_depth, want_rgb)
            else:
                assert _untouched(d), (want_depth, want_rgb)
            if want_rgb:
                assert R.same_image(c[:3 * n].reshape(want[1].shape), want[1]) and _untouched(c[3 * n:]), (want_depth, want_rgb)
            else:
                assert _untouched(c), (want_depth, want_rgb)
            got[(want_depth, want_rgb)] = (d[:n].reshape(want[0].shape), c[:3 * n].reshape(want[1].shape))
    finally:
        torch.cuda.synchronize()
        N.check(L.sdfk_set_stream(None))
    host = _host(rm)
    _check(host, want, size)
    assert R.same_image(got[(True, True)][0], host[0]) and R.same_image(got[(True, True)][1], host[1])
    assert R.same_image(got[(True, False)][0], host[0]) and R.same_image(got[(False, True)][1], host[1])


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(gpu):
    import torch
    rm = _marcher(S.readme_repeat_xy()[1], "oblique", size=(5, 4))
    good = _args(rm)

    def replaced(**kw):
        a = list(good)
        for k, v in kw.items():
            a[{"program": 0, "width": 1, "height": 2, "camera": 3, "matrix": 4, "iterations": 7}[k]] = v
        return a
    bad = {"width 0": replaced(width=0), "height 0": replaced(height=0), "negative iterations": replaced(iterations=-1),
           "null program": replaced(program=None), "null camera": replaced(camera=None), "null matrix": replaced(matrix=None),
           "negative width": replaced(width=-5), "more than 2^31 pixels": replaced(width=65536, height=32769)}
    L = N.lib()
    dev = torch.device("cuda:0")
    for what, a in bad.items():
        # (one-pixel buffers in the last case: it has to be refused before anything is allocated or launched)
        n = 1 if "2^31" in what else 20
        depth, rgb = np.full(n, GUARD, f32), np.full(3 * n, GUARD, f32)
        assert L.sdfk_raymarch(*a, depth.ctypes.data, rgb.ctypes.data) == N.ERR_INVALID, what
        assert L.sdfk_last_error(), what
        assert _untouched(depth) and _untouched(rgb), what
        dd, cd = torch.full((n,), float(GUARD), device=dev), torch.full((3 * n,), float(GUARD), device=dev)
        assert L.sdfk_raymarch_device(*a, C.c_void_p(dd.data_ptr()), C.c_void_p(cd.data_ptr())) == N.ERR_INVALID, what
        torch.cuda.synchronize()
        assert _untouched(dd.cpu().numpy()) and _untouched(cd.cpu().numpy()), what
    # ... and the arguments they were made from are good
    _check(_host(rm), R.catalogue_render("readme_repeat_xy", "oblique", size=(5, 4)), "5x4")


# ---- pinned destination ----------------------------------------------------------------------------------------------------------
def test_pinned_destination_equals_pageable(gpu):
    rm = _marcher(S.readme_repeat_xy()[1], "oblique", size=(255, 3), iterations=25)
    n = 255 * 3
    want = _host(rm)
    _check(want, R.catalogue_render("readme_repeat_xy", "oblique", size=(255, 3), iterations=25), "pageable")
    L = N.lib()
    block = C.c_void_p()
    N.check(L.sdfk_host_alloc(4 * (4 * n + 2), C.byref(block)))
    try:
        mem = np.ctypeslib.as_array((C.c_float * (4 * n + 2)).from_address(block.value))
        mem[:] = GUARD
        depth, rgb = mem[:n], mem[n + 1:4 * n + 1]       # (a guard float behind each)
        N.check(L.sdfk_raymarch(*_args(rm), depth.ctypes.data, rgb.ctypes.data))
        assert R.same_image(depth.reshape(want[0].shape), want[0]) and R.same_image(rgb.reshape(want[1].shape), want[1])
        assert mem[n] == GUARD and mem[4 * n + 1] == GUARD
        del depth, rgb, mem
    finally:
        L.sdfk_host_free(block)


# ---- the ray kernel's constants -----------------------------------------------------------------------------------------------------
def test_forty_radii_one_ray_module(gpu, tmp_path):
    """constants are kernel arguments in the ray kernel too (its own instantiation, PK_RAYMARCH): forty spheres of one structure
    cost ONE compile, and every image is the oracle's for that radius"""
    L = N.lib()
    N.check(L.sdfk_set_cache_dir(str(tmp_path / "jit").encode()))
    try:
        def sphere(r):
            # a structure no other test builds (`+ (y - y)` adds +0: the same values): the counters do not depend on what ran before
            return Sdf(lambda p: Vec4.of((0, 0, 0), (MathF.Sqrt((p.x * p.x + p.y * p.y) + p.z * p.z) - r) + (p.y - p.y)), False)

        c0, h0 = _jit()
        sources = set()
        for i in range(40):
            r = 0.5 + 0.0207 * i
            sdf = sphere(r)
            s = O.Scene(); s.sphere_w(r)
            want = R.render(s, "oblique")
            assert R.census(*want, 100.0)[2] >= 9, r      # (the sphere is in the picture: 9 .. 69 pixels)
            _check(_images(_marcher(sdf, "oblique")), want, r)
            sources.add(sdf.source())
        c1, h1 = _jit()
        assert len(sources) == 1 and "K.k[" in sources.pop()
        assert c1 - c0 == 1 and h1 - h0 == 0, "one ray kernel for the forty programs"
    finally:
        N.check(L.sdfk_set_cache_dir(None))


def test_constants_baked_as_literals_and_as_arguments(gpu):
    """RepeatX periods: 2.0 and 1.0 are literals (x / 2^k is a multiplication), 1.5 and 0.75 share one structure"""
    col = (0.25, 0.5, 0.75)
    src = {}
    for period in (2.0, 1.5, 1.0, 0.75):
        sdf = SdfExprs.Sphere(0.4375, col).RepeatX(period).ToSdf()
        scene = O.Scene()
        scene.f_repeat_x(scene.f_sphere(0.4375, col), period)
        for cam in ("oblique", "up_z"):
            want = R.render(scene, cam)
            assert R.census(*want, 100.0)[2] > 20, (period, cam)
            _check(_images(_marcher(sdf, cam)), want, (period, cam))
        src[period] = sdf.source()
    assert src[1.5] == src[0.75] and src[2.0] != src[1.5] and src[1.0] != src[1.5]


def _union3(sphere, box, cyl):
    """(oracle scene, product SDF) of Union(Sphere.Translate, Union(Box.Translate, Cylinder))"""
    (sr, sx), (bb, bx), (cr, ch) = sphere, box, cyl
    s = O.Scene()
    s.root = s.f_union(s.f_translate(s.f_sphere(sr), sx, 0, 0), s.f_union(s.f_translate(s.f_box(bb), bx, 0, 0), s.f_cylinder(cr, ch)))
    sdf = SdfExprs.Union(SdfExprs.Sphere(sr).Translate(sx, 0, 0), SdfExprs.Union(SdfExprs.Box(bb).Translate(bx, 0, 0), SdfExprs.Cylinder(cr, ch))).ToSdf()
    return s, sdf


def test_one_source_two_sets_of_constants(gpu):
    """the 3-primitive unions of test_programs_with_many_constants_keep_literals: one module, two argument blocks -- a ray kernel
    that read stale or misordered K.k[] would render the wrong union"""
    (sa, a), (sb, b) = _union3((0.6, -1.0), (0.5, 1.0), (0.4, 0.6)), _union3((0.55, -1.25), (0.45, 1.5), (0.35, 0.65))
    assert a.source() == b.source() and "K.k[" in a.source()
    for cam in ("oblique", "up_z", "along_x"):
        wa, wb = R.render(sa, cam), R.render(sb, cam)
        assert not np.array_equal(wa[0], wb[0]) and R.census(*wa, 100.0)[2] >= 20 and R.census(*wb, 100.0)[2] >= 20
        for _ in range(2):      # a, b, a, b: each launch carries its own constants
            _check(_images(_marcher(a, cam)), wa, ("a", cam))
            _check(_images(_marcher(b, cam)), wb, ("b", cam))


@pytest.mark.parametrize("c", [float("nan"), float("inf"), -float("inf"), -0.0, 1e-42, -1e-42], ids=str)
def test_special_constants_reach_the_ray_kernel(gpu, c):
    """NaN, infinities, -0 and denormals added to the distance arrive through the argument block (or as literals) unchanged:
    against the numpy model over the traced IR"""
    sdf = Sdf(lambda p, c=c: Vec4.of((0, 0, 0), (p.Length() - 1.25) + np.float32(c)), False)
    ops, out = trace(sdf.fn, False)
    assert any(np.array_equal(np.float32(op[5]).view(np.uint32), np.float32(c).view(np.uint32)) for op in ops), "the constant is in the IR"
    w, h = R.SWEEP_SIZE
    for iterations in (1, 40):
        rm = _marcher(sdf, "default", iterations=iterations)
        pos, vpi = rm.camera()
        want = M.raymarch(ops, out, False, (), w, h, pos, vpi, 1.0, 100.0, iterations)
        _check(_host(rm), want, (c, iterations))
        if np.isnan(c):
            assert np.isnan(want[0]).all()
        elif np.isinf(c):      # one step lands on the constant; further steps make NaN of it wherever inf - inf or 0 * inf occurs
            assert (want[0] == c).all() if iterations == 1 else not np.isfinite(want[0]).any()
        else:
            assert np.isfinite(want[0]).all() and (want[0] < 100).sum() > 20


# ---- random compositions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.RANDOM_SEEDS)
def test_random_compositions(gpu, seed):
    sdf = S.random_scene(seed, depth=R.random_depth(seed))[1]
    _check(_images(_marcher(sdf, "oblique", size=R.RANDOM_SIZE, iterations=R.RANDOM_ITERATIONS)), R.random_render(seed), seed)


# ---- IR programs from inside their bodies ---------------------------------------------------------------------------------------------
INSIDE_LENS = (60.0, 0.05, R.INF)


def _against_model(sdf, model, ops, out, volumes, what):
    rm = _marcher(sdf, "inside", INSIDE_LENS)
    pos, vpi = O.ray_camera(R.view("inside"), INSIDE_LENS[0], *R.SWEEP_SIZE, INSIDE_LENS[1], INSIDE_LENS[2])
    mirror = rm.camera()
    assert np.array_equal(mirror[0], pos) and np.array_equal(mirror[1], vpi)
    want = model.raymarch(ops, out, True, volumes, *R.SWEEP_SIZE, pos, vpi, INSIDE_LENS[1], INSIDE_LENS[2], 40)
    _check(_host(rm), want, what)
    return want


def test_mathops_scenes_from_inside(gpu):
    from tests.test_gpu_mathops import SCENES
    for name, fn in SCENES.items():
        ops, out = trace(fn, True)
        want = _against_model(Sdf(fn, True), M, ops, out, (), name)
        assert not np.isnan(want[0]).any(), name
    # the camera is inside the twist's and the smooth union's bodies: their distance there is negative
    for name in ("twist", "smooth_union"):
        ops, out = trace(SCENES[name], True)
        assert M.run(ops, out, f32([[0, 0, 0.25]]))[3][0] < 0, name


def test_bound_volume_from_inside(gpu):
    rng = np.random.default_rng(4)
    n = 24
    mn, mx = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)
    px, py, pz = VM.grid_points(mn, mx, n, n, n)
    vals = (np.sqrt(px * px + py * py + pz * pz) - f32(1)).astype(f32)
    cols = rng.uniform(0, 1, (n, n, n, 3)).astype(f32)
    vox = Voxels(vals, cols, mn, mx)
    for interpolate in (True, False):
        sdf = vox.ToSdf(interpolate)
        ops, out, _ = trace_bound(sdf.fn, sdf.writes_color)
        want = _against_model(sdf, VM, ops, out, [(vals, cols, mn, mx)], interpolate)
        assert (want[0] < 0).any() and not np.isnan(want[0]).any()      # (the first step from inside the sphere goes backwards)
