"""Case tables of the ray marcher's stress tests (tests/test_raymarch_cases.py on the CPU, tests/test_gpu_raymarch_stress.py and
tests/test_gpu_raymarch_cpp.py on the GPU, tests/test_raymarch.py for the camera arithmetic): cameras, lenses, iteration counts and
image shapes chosen for the paths of sdfk_raymarch (csrc/sample_codegen.h) and of its entry points (csrc/lib_volume.hip) --

  cameras   outside views, one with up = z, one INSIDE a solid (the depth marches backwards), one thousands of units away, and one
            whose up vector is parallel to the view direction (Cross(up, z) = 0: the whole matrix is NaN);
  lenses    fields of view of 1, 45, 60 and 170 degrees; a near plane of 0.1 and of 0.05 (the start `near - 0.1` is zero / negative);
            a far plane below every hit; far = +inf (the other branch of CreatePerspectiveFieldOfView);
  shapes    a 1-pixel dimension ((float)(width - 1) = 0: every ray is NaN, in the reference too), 2-pixel dimensions, pixel counts
            of 255, 256 and 258 around the 256-lane block, and a width / a height beyond 65 536.

Plain data and helpers: importable without a GPU."""
import functools

import numpy as np

from oracle import oracle as O

f32 = np.float32
INF = float("inf")

# name -> (position, target, up)
CAMERAS = {
    "default": ((0, 0, 5), (0, 0, 0), (0, 1, 0)),
    "oblique": ((-2, 2, 4), (0, 0, 0), (0, 1, 0)),
    "up_z": ((3, -1, 2.5), (0.2, 0.1, -0.3), (0, 0, 1)),
    "inside": ((0, 0, 0.25), (0, 0, -1), (0, 1, 0)),
    "along_x": ((6, 0, 0), (0, 0, 0), (0, 1, 0)),
    "far_away": ((0, 0, 5000), (0, 0, 0), (0, 1, 0)),
    "degenerate_up": ((0, 5, 0), (0, 0, 0), (0, 1, 0)),
}
# (vertical field of view in degrees, near, far)
DEFAULT_LENS = (60.0, 1.0, 100.0)
LENSES = [DEFAULT_LENS, (170.0, 1.0, 100.0), (1.0, 1.0, 100.0), (60.0, 0.1, 100.0), (60.0, 0.05, INF), (60.0, 1.0, 3.0), (45.0, 0.5, 250.0)]
ITERATIONS = [0, 1, 2, 40, 400]
# (width, height)
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 2), (2, 3), (128, 2), (2, 128), (85, 3), (86, 3), (255, 3), (70001, 2), (2, 70001)]

SWEEP_SCENES = ["union8", "readme_repeat_xy", "sdf_with_color", "plane_w"]
SWEEP_CAMERAS = ["default", "oblique", "up_z", "inside", "along_x"]      # the cameras whose images hold no NaN depth
SWEEP_SIZE = (33, 21)
# the catalogue scenes on which the C oracle and the numpy model of the traced IR are compared
MODEL_SCENES = ["readme_repeat_xy", "union8", "sdf_with_color", "plane_w", "cylinder", "repeat_xz_box", "box_w"]
# (camera, lens, iterations) of that comparison
MODEL_VIEWS = [("oblique", DEFAULT_LENS, 40), ("inside", (60.0, 0.05, INF), 40), ("up_z", DEFAULT_LENS, 400)]
RANDOM_SEEDS = range(16)
RANDOM_SIZE, RANDOM_ITERATIONS = (61, 37), 32


def random_depth(seed):
    """the depth of tests/scenes.py::random_scene for `seed`"""
    return 3 + seed % 2


def view(camera):
    """the oracle's look-at matrix of a camera of CAMERAS (by name) or of a (position, target, up) triple"""
    return O.look_at(*(CAMERAS[camera] if isinstance(camera, str) else camera))


def render(scene, camera, lens=DEFAULT_LENS, size=SWEEP_SIZE, iterations=40, **kw):
    """the oracle's (depth, rgb) of a scene graph"""
    fov, near, far = lens
    return O.raymarch(scene, size[0], size[1], view=view(camera), fov_degrees=fov, near=near, far=far, iterations=iterations, **kw)


def render_with(scene, pos, vpi, near, far, size, iterations):
    """the oracle's (depth, rgb) for a camera position and an inverse view-projection given as such: what sdfk_raymarch takes
    (the far plane of the sky test need not be the one the matrix was made with)"""
    import ctypes as C
    w, h = size
    depth, rgb = np.empty((h, w), f32), np.empty((h, w, 3), f32)
    O.lib().orc_raymarch(scene.carray(), scene.root, w, h, (C.c_float * 3)(*[float(x) for x in pos]),
                         (C.c_float * 16)(*[float(x) for x in np.asarray(vpi, f32).ravel()]), near, far, iterations,
                         depth.ctypes.data, rgb.ctypes.data, 0)
    return depth, rgb


def far_at_a_hit(name, camera="default", size=SWEEP_SIZE, iterations=40):
    """a far plane EXACTLY at the depth of a hit: (pos, vpi, far, depth, rgb) -- the camera of the default lens, the depth of the
    image's middle pixel as the far plane of the sky test `depth > far`, and the oracle's images for that far plane.  The pixels at
    exactly that depth are not sky; `>=` in place of `>` would paint them as sky."""
    from tests import scenes as S
    scene = S.CATALOGUE[name]()[0]
    pos, vpi = O.ray_camera(view(camera), DEFAULT_LENS[0], size[0], size[1], DEFAULT_LENS[1], DEFAULT_LENS[2])
    far = float(catalogue_render(name, camera, DEFAULT_LENS, size, iterations)[0][size[1] // 2, size[0] // 2])
    return (pos, vpi, far, *render_with(scene, pos, vpi, DEFAULT_LENS[1], far, size, iterations))


@functools.lru_cache(maxsize=None)
def catalogue_render(name, camera, lens=DEFAULT_LENS, size=SWEEP_SIZE, iterations=40):
    """the oracle's (depth, rgb) of tests/scenes.py::CATALOGUE[name], computed once per session and read-only"""
    from tests import scenes as S
    depth, rgb = render(S.CATALOGUE[name]()[0], camera, lens, size, iterations)
    depth.setflags(write=False)
    rgb.setflags(write=False)
    return depth, rgb


@functools.lru_cache(maxsize=None)
def random_render(seed):
    """the oracle's (depth, rgb) of random_scene(seed) from `oblique`, once per session and read-only"""
    from tests import scenes as S
    depth, rgb = render(S.random_scene(seed, depth=random_depth(seed))[0], "oblique", DEFAULT_LENS, RANDOM_SIZE, RANDOM_ITERATIONS)
    depth.setflags(write=False)
    rgb.setflags(write=False)
    return depth, rgb


def census(depth, rgb, far):
    """(NaN-depth pixels, sky pixels (depth > far), non-sky pixels (depth <= far: a NaN depth is neither), pixels with a NaN
    colour); rgb may be None (0 NaN colours)"""
    depth = np.asarray(depth)
    with np.errstate(invalid="ignore"):
        sky, hit = depth > f32(far), depth <= f32(far)
    nan_rgb = 0 if rgb is None else int(np.isnan(np.asarray(rgb)).any(axis=-1).sum())
    return int(np.isnan(depth).sum()), int(sky.sum()), int(hit.sum()), nan_rgb


def same_image(got, want):
    """whole images equal, NaN == NaN; where the reference is finite the sign bit too (-0.0 is not +0.0).  NaN payloads and NaN
    signs are not compared: x86 and the GPU differ there."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype or not np.array_equal(got, want, equal_nan=True):
        return False
    fin = np.isfinite(want)
    return bool(np.array_equal(np.signbit(got[fin]), np.signbit(want[fin])))
