"""The references of the ray marcher's stress tests, alone: the images of the C oracle (oracle/sdfk_oracle_ray.c) over the tables of
tests/raymarch_cases.py hold what the GPU tests need them to hold -- sky AND hits, backward marches, an all-sky frame, NaN colours
on sound depths, all-NaN frames exactly where the arithmetic says so -- so that no GPU comparison can pass on an image of nothing;
and the oracle agrees, bit for bit, with the numpy model of the traced IR (tests/mathops_model.py).  Every condition is asserted on
the reference's images, never on the GPU's.  The figures in the comments were measured with the oracle."""
import numpy as np
import pytest

from tests import raymarch_cases as R
from tests import scenes as S

f32 = np.float32


# ---- the case tables --------------------------------------------------------------------------------------------------------------
def test_tables():
    assert list(R.CAMERAS) == ["default", "oblique", "up_z", "inside", "along_x", "far_away", "degenerate_up"]
    assert len(R.LENSES) == 7 and R.LENSES[0] == R.DEFAULT_LENS == (60.0, 1.0, 100.0)
    assert R.ITERATIONS == [0, 1, 2, 40, 400]
    pixels = sorted(w * h for w, h in R.SHAPES)
    assert {255, 256, 258} <= set(pixels) and pixels[-1] == 140002 and max(max(s) for s in R.SHAPES) > 65536
    assert sum(1 for w, h in R.SHAPES if min(w, h) == 1) == 3


def test_census_counts():
    depth = f32([[1.0, 101.0, np.nan], [np.inf, -np.inf, 100.0]])
    rgb = np.zeros((2, 3, 3), f32)
    rgb[0, 1, 2] = np.nan
    rgb[1, 0] = np.nan
    assert R.census(depth, rgb, 100.0) == (1, 2, 3, 2)
    assert R.census(depth, None, np.inf) == (1, 0, 5, 0)
    assert R.same_image(f32([0.0, np.nan]), f32([0.0, np.nan])) and not R.same_image(f32([-0.0]), f32([0.0]))
    assert not R.same_image(f32([1.0]), f32([np.nan])) and not R.same_image(f32([1.0]), f32([[1.0]]))


# ---- camera sweep -----------------------------------------------------------------------------------------------------------------
def test_camera_sweep_has_no_nan_depth_and_mostly_sky_and_hits():
    both = 0
    for name in R.SWEEP_SCENES:
        for cam in R.SWEEP_CAMERAS:
            depth, rgb = R.catalogue_render(name, cam)
            nan, sky, hit, _ = R.census(depth, rgb, 100.0)
            assert nan == 0, (name, cam)
            both += sky > 0 and hit > 0
    assert both >= 12, both     # measured: 14 of 20


@pytest.mark.parametrize("iterations", R.ITERATIONS)
def test_degenerate_up_is_all_nan(iterations):
    """up parallel to the view direction: Cross(up, z) = 0, Normalize divides 0 by 0, x and y of the view are NaN and every
    entry of its inverses.  Without a step the depth is still `near - 0.1`.  A box swallows the NaN: Vector3.Max(wd, 0) and
    Min(wd, 0) of a NaN point are 0, so its distance is 0 and the depth of the two scenes with a box (union8 takes
    `a.W < b.W ? a : b` = its last box) never leaves `near - 0.1`; their colour is NaN all the same."""
    assert np.isnan(R.view("degenerate_up")[:3, :2]).all()
    for name in R.SWEEP_SCENES:
        depth, rgb = R.catalogue_render(name, "degenerate_up", iterations=iterations)
        if iterations == 0 or name in ("union8", "sdf_with_color"):
            assert np.array_equal(depth, np.full(depth.shape, f32(1.0) - f32(0.1), f32)), name
        else:
            assert np.isnan(depth).all(), name
        assert np.isnan(rgb).all(), name      # (the shading point is NaN either way)


def test_far_away_camera_sees_the_scene_as_sky_or_hit():
    for name in R.SWEEP_SCENES:
        depth, rgb = R.catalogue_render(name, "far_away")
        assert not np.isnan(depth).any() and np.abs(depth).max() > 100.0, name


# ---- single conditions ------------------------------------------------------------------------------------------------------------
def test_backward_marching_inside_a_solid():
    depth, _ = R.catalogue_render("sdf_with_color", "inside", (60.0, 0.1, 100.0))
    assert (depth < 0).all() and depth.min() >= f32(-0.08) and depth.max() <= f32(-0.04)     # measured: -0.073 .. -0.05


def test_far_plane_below_the_hits_is_all_sky():
    depth, rgb = R.catalogue_render("readme_repeat_xy", "default", (60.0, 1.0, 3.0))
    assert depth.min() >= f32(4.4)                                                            # measured: from 4.5
    assert R.census(depth, rgb, 3.0) == (0, depth.size, 0, 0)
    assert np.array_equal(rgb, np.broadcast_to(f32([0.5, 0.75, 1.0]), rgb.shape))
    # ... and with the default far plane the same frame has hits: the far plane is what makes the sky
    depth, rgb = R.catalogue_render("readme_repeat_xy", "default")
    assert R.census(depth, rgb, 100.0)[2] > 0


@pytest.mark.parametrize("name", ["plane_w", "sdf_with_color", "union8"])
def test_far_plane_exactly_at_a_depth(name):
    """the sky test is `depth > far`, not `>=`: with the far plane at the depth of the middle pixel that pixel is not sky, deeper
    ones are, and its colour is a lit one, not the sky's"""
    pos, vpi, far, depth, rgb = R.far_at_a_hit(name)
    nan, sky, hit, nan_rgb = R.census(depth, rgb, far)
    at = depth == f32(far)
    assert nan == 0 and sky > 0 and hit >= at.sum() >= 1, (sky, hit, int(at.sum()))
    assert np.array_equal(depth, R.catalogue_render(name, "default")[0])      # (the far plane does not touch the depth)
    assert not (rgb[at] == f32([0.5, 0.75, 1.0])).all(axis=-1).any() and (rgb[depth > f32(far)] == f32([0.5, 0.75, 1.0])).all()
    # no step at all, far at the near start: nothing is sky
    lens = (60.0, 1.0, float(f32(1.0) - f32(0.1)))
    depth, rgb = R.catalogue_render(name, "default", lens, iterations=0)
    assert (depth == f32(lens[2])).all() and R.census(depth, rgb, lens[2])[1:3] == (0, depth.size)
    assert np.array_equal(rgb, np.full(rgb.shape, f32(0.1), f32))


def test_far_infinity_has_no_sky():
    for name in R.SWEEP_SCENES:
        for cam in ("oblique", "inside"):
            depth, rgb = R.catalogue_render(name, cam, (60.0, 0.05, R.INF))
            assert R.census(depth, rgb, R.INF)[1] == 0, (name, cam)
            assert not np.array_equal(rgb, np.broadcast_to(f32([0.5, 0.75, 1.0]), rgb.shape)), (name, cam)


def test_nan_colour_on_a_sound_depth():
    """400 steps: the sky rays have run off to +inf, `inf * 0` makes their colour NaN, and no depth is NaN"""
    depth, rgb = R.catalogue_render("union8", "up_z", iterations=400)
    nan, sky, hit, nan_rgb = R.census(depth, rgb, 100.0)
    assert nan == 0 and np.isposinf(depth).any()
    assert sky > 0 and hit > 0 and sky + hit == depth.size == 693
    assert np.array_equal(np.isnan(rgb).any(axis=-1), depth > 100.0) and nan_rgb == sky      # measured: 444 of 693
    assert np.array_equal(np.isposinf(depth), depth > 100.0)


# ---- image shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(shape):
    depth, rgb = R.catalogue_render("readme_repeat_xy", "oblique", size=shape, iterations=25)
    assert depth.shape == shape[::-1] and rgb.shape == shape[::-1] + (3,)
    if min(shape) == 1:      # (float)(n - 1) = 0: 0 / 0 in a ray coordinate of every pixel
        assert np.isnan(depth).all() and np.isnan(rgb).all()
        return
    nan, sky, hit, nan_rgb = R.census(depth, rgb, 100.0)
    assert nan == 0 and nan_rgb == 0 and hit >= 4, (nan, sky, hit, nan_rgb)
    if shape == (70001, 2):
        assert (sky, hit) == (69994, 70008)


# ---- random compositions ----------------------------------------------------------------------------------------------------------
def test_random_compositions_are_in_the_picture():
    seen = 0
    for seed in R.RANDOM_SEEDS:
        depth, rgb = R.random_render(seed)
        nan, sky, hit, nan_rgb = R.census(depth, rgb, 100.0)
        assert nan == 0 and nan_rgb == 0, seed
        seen += hit >= 200
    assert seen >= 10, seen      # measured: 12


# ---- the two references agree -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.MODEL_SCENES)
def test_oracle_equals_the_model_of_the_traced_program(name):
    from oracle import oracle as O
    from sdfkit_amd.expr import trace
    from tests import mathops_model as M
    sdf = S.CATALOGUE[name]()[1]
    ops, out = trace(sdf.fn, sdf.writes_color)
    w, h = R.SWEEP_SIZE
    for cam, lens, iterations in R.MODEL_VIEWS:
        depth, rgb = R.catalogue_render(name, cam, lens, R.SWEEP_SIZE, iterations)
        pos, vpi = O.ray_camera(R.view(cam), lens[0], w, h, lens[1], lens[2])
        md, mrgb = M.raymarch(ops, out, sdf.writes_color, (), w, h, pos, vpi, lens[1], lens[2], iterations)
        assert R.same_image(md, depth), (name, cam)
        assert R.same_image(mrgb, rgb), (name, cam)
