"""The cases of the depth-fusion tests (tests/test_depth_fusion_host.py on the CPU, tests/test_gpu_depth_fusion*.py on the device):
volumes with frames to integrate, and frames to unproject; the runners of the numpy model (tests/depth_fusion_model.py) and of the
host program (tests/cpp/depth_fusion_host.cpp) over them.  Shapes are the smallest that can go wrong: nz not a multiple of the
four voxels a lane takes, a row longer than a 256-lane block, a slab, images of one pixel, pixel counts around the scan's blocks."""
import functools
import os
import struct
import subprocess

import numpy as np

from tests import depth_fusion_model as M

f32, u32, i32, i64 = np.float32, np.uint32, np.int32, np.int64
INF, NAN = np.inf, np.nan
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
OUTSIDE = ((1.6, 1.1, 2.9), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
SPHERE = (((0.0, 0.0, 0.0), 0.6),)


def camera(width, height, cam, **lens):
    """(position, view_projection, view_projection_inverse, near, far) of the library's own host arithmetic"""
    from sdfkit_amd.fusion import Camera
    return Camera(width, height, cam, **lens)


def frame(depth, cam=OUTSIDE, lens=None, depth_min=None, depth_max=None, weight=1.0, carve=True):
    """One frame of a volume case: the image (height, width), its camera and lens, and the call's own arguments."""
    lens = lens or {}
    height, width = depth.shape
    pos, vp, vpi, near, far = camera(width, height, cam, **lens)
    return {"depth": np.ascontiguousarray(depth, f32), "cam": cam, "lens": lens, "pos": pos, "vp": vp, "vpi": vpi,
            "depth_min": f32(near if depth_min is None else depth_min), "depth_max": f32(far if depth_max is None else depth_max),
            "weight": f32(weight), "flags": M.CARVE_BEYOND if carve else 0}


def scene_depth(width, height, cam=OUTSIDE, lens=None, spheres=SPHERE):
    pos, _, vpi, _, _ = camera(width, height, cam, **(lens or {}))
    return M.sphere_depth(width, height, pos, vpi, spheres)


def volume(shape, frames, box=UNIT, truncation=0.25, max_weight=INF, fill=None, weights=None, z0=0, nz_global=None):
    shape = tuple(shape)
    D0 = np.full(shape, -truncation if fill is None else fill, f32) if not isinstance(fill, np.ndarray) else fill.astype(f32)
    W0 = np.zeros(shape, f32) if weights is None else weights.astype(f32)
    return {"shape": shape, "mn": box[0], "mx": box[1], "truncation": f32(truncation), "max_weight": f32(max_weight), "D0": D0, "W0": W0,
            "z0": z0, "nz_global": shape[2] if nz_global is None else nz_global, "frames": frames}


def pattern(width, height, kind, value=3.0, other=INF):
    d = np.full((height, width), value, f32)
    if kind == "none":
        d[:] = other
    elif kind == "alternating":
        d.reshape(-1)[1::2] = other
    return d


def odd_depths(width, height, depth_max):
    """A sphere frame with every kind of pixel sprinkled in: NaN, 0, negative, +inf, depth_max exactly and just beyond it."""
    d = scene_depth(width, height).copy()
    odd = np.array([NAN, 0.0, -1.0, INF, depth_max, np.nextafter(f32(depth_max), f32(INF)), -INF, np.nextafter(f32(depth_max), f32(0))], f32)
    flat = d.reshape(-1)
    k = np.arange(0, len(flat), 3)
    flat[k] = odd[np.arange(len(k)) % len(odd)]
    return d


def seeded_weights(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0.0, -0.0, -1.0, NAN, 1.5, 3.0, 0.25], f32), size=shape).astype(f32)


def seeded_values(shape, seed):
    """finite values: where the weight is positive they enter the average"""
    return np.random.default_rng(seed).uniform(-0.25, 0.25, shape).astype(f32)


def _exact_axis():
    """The camera on the z axis looking down it, everything exactly representable: cell centres x, y in {-1, -.5, 0, .5, 1}, z in
    -.875 .. .875 by .25.  On the column x = y = 0: c_0 = c_1 = 0, so u = v = 1.5 and u + .5 = 2 exactly (the tie goes to pixel 2),
    r = 4 - z, and with the pixel's depth 4: s = z, which is -truncation exactly at z = -.375 (kept: only s < -truncation is
    skipped), beyond it at -.625 (skipped), and +truncation exactly at z = .375 (a surface observation within the truncation)."""
    d = (4.0 + 0.0625 * (1 + np.arange(16))).reshape(4, 4).astype(f32)
    d[2, 2] = 4.0
    fr = frame(d, ((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), carve=False)
    return volume((5, 5, 8), [fr], box=((-1.25, -1.25, -1.0), (1.25, 1.25, 1.0)), truncation=0.375)


def _sequence(max_weight=INF, weight=1.0):
    cams = [OUTSIDE, ((-2.5, 0.4, 1.9), (0, 0, 0), (0, 1, 0)), ((0.3, 3.1, 0.5), (0, 0, 0), (0, 0, 1)), ((0.2, -0.4, -3.2), (0, 0, 0), (0, 1, 0))]
    frames = [frame(scene_depth(64, 48, c), c, weight=weight, depth_max=6.0) for c in cams] * 2
    return volume((9, 10, 11), frames, max_weight=max_weight)


VOLUMES = {}
for _shape in ((5, 6, 7), (3, 2, 9), (2, 3, 261), (33, 17, 12)):
    for _carve in (True, False):
        VOLUMES["sphere_%dx%dx%d_%s" % (_shape + ("carve" if _carve else "open",))] = (
            lambda s=_shape, c=_carve: volume(s, [frame(scene_depth(64, 48), carve=c, depth_max=6.0)], fill=None if c else 0.25))
for _w, _h in ((1, 1), (2, 2), (3, 5)):
    for _kind in ("all", "none", "alternating"):
        VOLUMES[f"image_{_w}x{_h}_{_kind}"] = lambda w=_w, h=_h, k=_kind: volume((5, 6, 7), [frame(pattern(w, h, k), depth_max=6.0)])
VOLUMES["image_3x5_none_open"] = lambda: volume((5, 6, 7), [frame(pattern(3, 5, "none"), depth_max=6.0, carve=False)], fill=0.25)
VOLUMES["slab"] = lambda: volume((6, 5, 5), [frame(scene_depth(64, 48), depth_max=6.0)], z0=3, nz_global=12)
VOLUMES["slab_whole"] = lambda: volume((6, 5, 12), [frame(scene_depth(64, 48), depth_max=6.0)])
VOLUMES["camera_inside"] = lambda: volume((9, 8, 10), [frame(pattern(64, 48, "alternating", 0.5), ((0.1, 0.05, -0.2), (1.0, 0.5, 0.3), (0, 1, 0)),
                                                             {"nearPlaneDistance": 0.125}, depth_max=2.0)])
VOLUMES["camera_at_cell_centre"] = lambda: volume((8, 8, 8), [frame(pattern(3, 5, "all", 0.5), ((0.125, 0.125, 0.125), (1.0, 1.0, 1.0), (0, 1, 0)),
                                                                     {"nearPlaneDistance": 0.125}, depth_max=2.0)])
VOLUMES["exact_axis"] = _exact_axis
VOLUMES["frustum_misses"] = lambda: volume((5, 6, 7), [frame(pattern(3, 5, "alternating"), ((0, 0, 5.0), (0, 0, 10.0), (0, 1, 0)), depth_max=6.0)],
                                           fill=np.arange(0x7fc00001, 0x7fc00001 + 210, dtype=u32).view(f32).reshape(5, 6, 7),
                                           weights=seeded_weights((5, 6, 7), 5))
for _carve in (True, False):
    VOLUMES["odd_depths_" + ("carve" if _carve else "open")] = lambda c=_carve: volume((9, 10, 11), [frame(odd_depths(64, 48, 3.5), carve=c,
                                                                                                             depth_max=3.5)])
VOLUMES["sequence"] = _sequence
VOLUMES["sequence_max_weight"] = lambda: _sequence(max_weight=2.5)
VOLUMES["sequence_weight_half"] = lambda: _sequence(max_weight=1.25, weight=0.5)
VOLUMES["seeded_weights"] = lambda: volume((9, 10, 11), [frame(scene_depth(64, 48), depth_max=6.0)], fill=seeded_values((9, 10, 11), 2),
                                           weights=seeded_weights((9, 10, 11), 3), max_weight=3.25)

NOTHING_WRITTEN = ("frustum_misses", "image_3x5_none_open")   # (with carving a frame without a valid pixel frees what it sees)


@functools.lru_cache(maxsize=None)
def volume_case(name):
    return VOLUMES[name]()


@functools.lru_cache(maxsize=None)
def volume_model(name):
    """-> (D, W, [stats of every frame]) after the case's frames"""
    c = volume_case(name)
    D, W, stats = c["D0"], c["W0"], []
    for fr in c["frames"]:
        D, W, st = M.integrate(D, W, c["mn"], c["mx"], fr["depth"], fr["pos"], fr["vp"], c["truncation"], fr["depth_min"], fr["depth_max"],
                               fr["weight"], c["max_weight"], fr["flags"], c["z0"], c["nz_global"])
        stats.append(st)
    return D, W, stats


# ---- frames to unproject: (width, height, pattern) -------------------------------------------------------------------------------
def _unproject(width, height, kind, rgb=True, cam=OUTSIDE):
    if kind == "scene":
        d = scene_depth(width, height, cam)
    else:
        d = pattern(width, height, kind, 3.0, INF)
        if kind == "alternating":   # every kind of invalid pixel
            flat = d.reshape(-1)
            bad = np.array([INF, NAN, 0.0, -2.0, 100.5], f32)
            flat[1::2] = bad[np.arange(len(flat[1::2])) % len(bad)]
    pos, _, vpi, near, far = camera(width, height, cam)
    k = np.arange(width * height, dtype=f32)
    colors = np.stack([k, k * f32(0.5), -k], -1).reshape(height, width, 3).astype(f32) if rgb else None
    return {"depth": d, "rgb": colors, "cam": cam, "pos": pos, "vpi": vpi, "depth_min": f32(near), "depth_max": f32(far), "width": width, "height": height}


FRAMES = {}
for _w, _h in ((1, 1), (2, 2), (3, 5), (64, 48), (51, 5), (16, 16), (257, 1), (1, 257), (65537, 1), (241, 272)):
    for _kind in ("all", "none", "alternating"):
        FRAMES[f"{_w}x{_h}_{_kind}"] = lambda w=_w, h=_h, k=_kind: _unproject(w, h, k)
FRAMES["scene_64x48"] = lambda: _unproject(64, 48, "scene")
FRAMES["scene_no_rgb"] = lambda: _unproject(33, 21, "scene", rgb=False)


@functools.lru_cache(maxsize=None)
def frame_case(name):
    return FRAMES[name]()


@functools.lru_cache(maxsize=None)
def frame_model(name):
    c = frame_case(name)
    return M.unproject(c["depth"], c["pos"], c["vpi"], c["depth_min"], c["depth_max"], c["rgb"])


def same_f32(a, b):
    """Equal as bits, a NaN that arithmetic made equal to any NaN (IEEE 754 leaves its sign and payload open)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u32)[~na], b.view(u32)[~nb]))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(np.array_equal(a.view(u32), b.view(u32)))


# ---- the refusals of both entry points, as depth_fusion.h decides them: name -> (changes to a good call, a word of the message) ---
GOOD = {"truncation": 0.25, "depth_min": 1.0, "depth_max": 100.0, "weight": 1.0, "max_weight": INF, "flags": 1, "width": 4, "height": 3,
        "a": {"shape": (4, 5, 6), "nz_global": 6, "z0": 0, "mn": (-1, -1, -1), "mx": (1, 1, 1), "storage": 1},
        "b": {"shape": (4, 5, 6), "nz_global": 6, "z0": 0, "mn": (-1, -1, -1), "mx": (1, 1, 1), "storage": 1}}
REFUSALS = {
    "width_0": ({"width": 0}, "width"), "height_negative": ({"height": -3}, "height"),
    "pixels_2_31": ({"width": 1 << 16, "height": 1 << 15}, "2^31"),
    "truncation_0": ({"truncation": 0.0}, "truncation"), "truncation_negative": ({"truncation": -1.0}, "truncation"),
    "truncation_inf": ({"truncation": INF}, "truncation"), "truncation_nan": ({"truncation": NAN}, "truncation"),
    "weight_0": ({"weight": 0.0}, "weight"), "weight_negative": ({"weight": -1.0}, "weight"), "weight_inf": ({"weight": INF}, "weight"),
    "weight_nan": ({"weight": NAN}, "weight"),
    "max_weight_nan": ({"max_weight": NAN}, "max_weight"), "max_weight_below": ({"max_weight": 0.5}, "max_weight"),
    "depth_min_nan": ({"depth_min": NAN}, "NaN"), "depth_max_nan": ({"depth_max": NAN}, "NaN"),
    "range_reversed": ({"depth_min": 2.0, "depth_max": 1.0}, "depth_min"),
    "flag_bits": ({"flags": 2}, "flag"), "flag_bits_high": ({"flags": 1 | (1 << 30)}, "flag"),
    "shape": ({"b": dict(GOOD["b"], shape=(4, 5, 7), nz_global=7)}, "shape"),
    "slab": ({"b": dict(GOOD["b"], z0=1, nz_global=7)}, "slab"),
    "box": ({"b": dict(GOOD["b"], mx=(1, 1, 1.5))}, "box"),
    "no_storage": ({"a": dict(GOOD["a"], storage=0)}, "storage"),
}
ACCEPTED = {"good": {}, "max_weight_equal": {"max_weight": 1.0}, "range_point": {"depth_min": 2.0, "depth_max": 2.0}, "no_flags": {"flags": 0},
            "huge_image": {"width": (1 << 16) - 1, "height": 1 << 15}}


def _refusal_record(changes):
    c = dict(GOOD, **changes)
    vols = b"".join(struct.pack("<5i6fi", *v["shape"], v["nz_global"], v["z0"], *v["mn"], *v["mx"], v["storage"]) for v in (c["a"], c["b"]))
    return struct.pack("<5f3i", c["truncation"], c["depth_min"], c["depth_max"], c["weight"], c["max_weight"], c["flags"], c["width"], c["height"]) + vols


# ---- the host program (tests/cpp/depth_fusion_host.cpp): the header's functions on the CPU ----------------------------------------
def build_host(directory, sanitize=False):
    exe = os.path.join(str(directory), "depth_fusion_host" + ("_san" if sanitize else ""))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall"] + extra +
                          [os.path.join(ROOT, "tests", "cpp", "depth_fusion_host.cpp"), "-o", exe])
    return exe


def _run_host(exe, mode, blob, directory, tag):
    src, dst = os.path.join(str(directory), f"{tag}.in"), os.path.join(str(directory), f"{tag}.out")
    with open(src, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "depth fusion ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    with open(dst, "rb") as f:
        return f.read()


def host_integrate(exe, directory, name):
    """The case's frames through the host program -> (D, W, [stats])"""
    c = volume_case(name)
    D, W, stats = c["D0"], c["W0"], []
    nx, ny, nz = c["shape"]
    for k, fr in enumerate(c["frames"]):
        h, w = fr["depth"].shape
        blob = struct.pack("<8q5f", nx, ny, nz, c["nz_global"], c["z0"], w, h, fr["flags"], c["truncation"], fr["depth_min"], fr["depth_max"],
                           fr["weight"], c["max_weight"]) + np.asarray(c["mn"], f32).tobytes() + np.asarray(c["mx"], f32).tobytes() + \
            np.asarray(fr["pos"], f32).tobytes() + np.asarray(fr["vp"], f32).tobytes() + fr["depth"].tobytes() + \
            np.ascontiguousarray(D, f32).tobytes() + np.ascontiguousarray(W, f32).tobytes()
        out = _run_host(exe, "integrate", blob, directory, f"{name}_{k}")
        stats.append([int(x) for x in np.frombuffer(out, i64, 4)])
        n = nx * ny * nz
        D = np.frombuffer(out, f32, n, 32).reshape(c["shape"])
        W = np.frombuffer(out, f32, n, 32 + 4 * n).reshape(c["shape"])
    return D, W, stats


def host_unproject(exe, directory, name):
    c = frame_case(name)
    rgb = c["rgb"]
    blob = struct.pack("<3q2f", c["width"], c["height"], int(rgb is not None), c["depth_min"], c["depth_max"]) + np.asarray(c["pos"], f32).tobytes() + \
        np.asarray(c["vpi"], f32).tobytes() + c["depth"].tobytes() + (b"" if rgb is None else rgb.tobytes())
    out = _run_host(exe, "unproject", blob, directory, name)
    n = int(np.frombuffer(out, i64, 1)[0])
    pts = np.frombuffer(out, f32, 3 * n, 8).reshape(n, 3)
    cols = np.frombuffer(out, f32, 3 * n, 8 + 12 * n).reshape(n, 3) if rgb is not None else None
    pix = np.frombuffer(out, i32, n, 8 + (24 if rgb is not None else 12) * n)
    return pts, cols, pix


def host_refusals(exe, directory, table):
    """name -> the message of depth_fusion.h ("" when accepted) for a table of changes to the good call"""
    names = list(table)
    blob = b"".join(_refusal_record(table[n][0] if isinstance(table[n], tuple) else table[n]) for n in names)
    lines = _run_host(exe, "refusals", blob, directory, "refusals").decode().split("\n")
    assert len(lines) >= len(names)
    return dict(zip(names, lines))
