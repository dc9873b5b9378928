"""CPU proof of depth fusion and unprojection (sdfkit_amd/csrc/depth_fusion.h, the very functions the kernels of lib_fusion.hip run,
built with g++ -O2 -ffp-contract=off by tests/cpp/depth_fusion_host.cpp) against the numpy model (tests/depth_fusion_model.py): every
case of tests/depth_fusion_cases.py bit for bit; what the hand-made cases are built to show; the refusals depth_fusion.h decides
(a NULL argument and values == weights are the entry points' own: tests/test_gpu_depth_fusion.py); the same program once more under
-fsanitize=address,undefined (a stand-alone program: nothing is preloaded); the entry points exported and refusing to run without
a device; the accuracy of a closed scan through the model, recorded in tests/golden/depth_fusion_accuracy.json; and the
unprojected points of a model-rendered frame against that render's hit points."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sdfkit_amd import _native as N
from tests import depth_fusion_cases as Cs
from tests import depth_fusion_model as M

f32, u32 = np.float32, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_fusion_accuracy.json")
ENTRY_POINTS = ("sdfk_volume_integrate_depth", "sdfk_volume_integrate_depth_device", "sdfk_depth_unproject", "sdfk_depth_unproject_device")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_fusion")
    return Cs.build_host(d), d


@pytest.mark.parametrize("name", list(Cs.VOLUMES))
def test_integrate_equals_model(host, name):
    exe, d = host
    D, W, stats = Cs.volume_model(name)
    hD, hW, hstats = Cs.host_integrate(exe, d, name)
    assert hstats == stats
    assert Cs.bits_equal(hD, D) and Cs.bits_equal(hW, W)


@pytest.mark.parametrize("name", list(Cs.FRAMES))
def test_unproject_equals_model(host, name):
    exe, d = host
    pts, cols, pix = Cs.frame_model(name)
    hp, hc, hx = Cs.host_unproject(exe, d, name)
    assert np.array_equal(hx, pix) and Cs.same_f32(hp, pts)
    assert (cols is None and hc is None) or Cs.bits_equal(hc, cols)


def test_what_the_cases_are_built_to_show():
    m, c = Cs.volume_model, Cs.volume_case
    for name in Cs.VOLUMES:   # every frame of every case but the ones built to write nothing updates something
        assert all((st[0] > 0) == (name not in Cs.NOTHING_WRITTEN) for st in m(name)[2]), name
    for name in Cs.NOTHING_WRITTEN:
        assert Cs.bits_equal(m(name)[0], c(name)["D0"]) and Cs.bits_equal(m(name)[1], c(name)["W0"])
    # carving updates more voxels than the surface observations alone, and sees the same surface
    for shape in ("5x6x7", "3x2x9", "2x3x261", "33x17x12"):
        a, b = m(f"sphere_{shape}_carve")[2][0], m(f"sphere_{shape}_open")[2][0]
        assert a[0] > b[0] > 0 and a[1] == b[1] > 0 and a[3] == b[3]
    # a slab is the same planes of the whole volume
    D, W, st = m("slab")
    Dw, Ww, stw = m("slab_whole")
    assert Cs.bits_equal(D, Dw[:, :, 3:8]) and Cs.bits_equal(W, Ww[:, :, 3:8]) and 0 < st[0][0] < stw[0][0]
    # the camera inside the box: voxels behind it (c_3 <= 0) are skipped, voxels in front are seen
    ci = c("camera_inside")
    p = M.centres(ci["mn"], ci["mx"], ci["shape"])
    vp = ci["frames"][0]["vp"].reshape(-1)
    c3 = ((p[0] * vp[3] + p[1] * vp[7]) + p[2] * vp[11]) + vp[15]
    changed = m("camera_inside")[1] != ci["W0"]
    assert (c3 <= 0).sum() > 100 and not changed[c3 <= 0].any() and changed.sum() > 20
    # the camera at a cell centre: that voxel has r = 0 and c_3 = 0 exactly, and is skipped
    cc = c("camera_at_cell_centre")
    p = M.centres(cc["mn"], cc["mx"], cc["shape"])
    at = (p[0] == f32(0.125)) & (p[1] == f32(0.125)) & (p[2] == f32(0.125))
    assert at.sum() == 1 and m("camera_at_cell_centre")[1][at] == 0 and m("camera_at_cell_centre")[2][0][0] > 0
    # the exact ties on the column x = y = 0 (ix = iy = 2), whose pixel is (2, 2) with depth 4: z = -.875 .. .875
    D, W, _ = m("exact_axis")
    col_d, col_w = D[2, 2], W[2, 2]
    z = (f32(-0.875) + np.arange(8).astype(f32) * f32(0.25)).astype(f32)
    assert col_w.tolist() == [0, 0, 1, 1, 1, 1, 1, 1]               # s = z: -.875 and -.625 are beyond -truncation, -.375 is ON it
    assert col_d[2] == f32(-0.375) and col_d[5] == f32(0.375) and col_d[6] == f32(0.375) and np.array_equal(col_d[2:6], z[2:6])
    assert col_d[0] == f32(-0.375)                                   # (unseen: the fill)
    # every kind of depth: the carved run updates where the open one cannot, and both count the valid pixels alike
    a, b = m("odd_depths_carve")[2][0], m("odd_depths_open")[2][0]
    assert a[0] > b[0] > 0 and a[3] == b[3] and a[1] == b[1]
    # weights: the cap is reached and holds; a weight of one half; user-seeded weights with zeros, negatives and NaN count as unseen
    W = m("sequence")[1]
    Wc = m("sequence_max_weight")[1]
    assert W.max() > 2.5 and Wc.max() == f32(2.5) and np.array_equal(Wc, np.minimum(W, f32(2.5)))
    assert not Cs.bits_equal(m("sequence")[0], m("sequence_max_weight")[0])
    assert m("sequence_weight_half")[1].max() == f32(1.25) and set(np.unique(m("sequence_weight_half")[1]).tolist()) <= {0.0, 0.5, 1.0, 1.25}
    sw = c("seeded_weights")
    D, W, st = m("seeded_weights")
    unseen = ~(sw["W0"] > 0)
    upd = ~Cs_bits_same(W, sw["W0"])
    assert st[0][2] == (upd & unseen).sum() > 50 and np.isnan(sw["W0"]).sum() > 50 and (sw["W0"] < 0).sum() > 50
    assert np.all(W[upd & unseen] == 1) and np.all(np.abs(D[upd & unseen]) <= f32(0.25)) and np.nanmax(W) == f32(3.25)
    # unprojection: images of width or height one have non-finite rays
    assert not np.isfinite(Cs.frame_model("257x1_all")[0]).any() and np.isfinite(Cs.frame_model("241x272_all")[0]).all()
    assert len(Cs.frame_model("65537x1_alternating")[2]) == 32769 and len(Cs.frame_model("16x16_none")[2]) == 0


def Cs_bits_same(a, b):
    return np.ascontiguousarray(a, f32).view(u32) == np.ascontiguousarray(b, f32).view(u32)


def test_refusals(host):
    exe, d = host
    said = Cs.host_refusals(exe, d, Cs.REFUSALS)
    for name, (_, word) in Cs.REFUSALS.items():
        assert said[name] and word in said[name], (name, said[name])
    assert all(v == "" for v in Cs.host_refusals(exe, d, Cs.ACCEPTED).values())


def test_host_program_under_sanitizers(tmp_path):
    exe = Cs.build_host(tmp_path, sanitize=True)
    for name in ("sphere_2x3x261_carve", "image_1x1_all", "camera_at_cell_centre", "exact_axis", "odd_depths_carve", "frustum_misses", "slab"):
        D, W, stats = Cs.volume_model(name)
        hD, hW, hstats = Cs.host_integrate(exe, tmp_path, name)
        assert hstats == stats and Cs.bits_equal(hD, D) and Cs.bits_equal(hW, W), name
    for name in ("1x1_all", "257x1_alternating", "scene_64x48", "scene_no_rgb"):
        assert np.array_equal(Cs.host_unproject(exe, tmp_path, name)[2], Cs.frame_model(name)[2]), name
    assert Cs.host_refusals(exe, tmp_path, Cs.REFUSALS)["box"]


# ---- the C ABI ----
def test_entry_points_exported():
    L = N.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in N.SIGNATURES, name
    assert C.sizeof(N.FusionParams) == 24


def test_refuse_without_device():
    """No device (or sdfk_init not called): every new entry point returns SDFK_ERR_NO_DEVICE, in a fresh process."""
    p = subprocess.run([sys.executable, "-c", "from tests.test_depth_fusion_host import _no_device; _no_device(); print('refusals ok')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "refusals ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def _no_device():
    L = N.lib()
    a = np.full(16, 2.0, f32)
    A = C.c_void_p(a.ctypes.data)
    cam, m = N.f3((0, 0, 5)), (C.c_float * 16)(*([1.0] * 16))
    prm = N.FusionParams(0.25, 1.0, 100.0, 1.0, np.inf, 1)
    n, st = C.c_int64(-7), (C.c_int64 * 4)(-7, -7, -7, -7)
    calls = {
        "sdfk_volume_integrate_depth": lambda: L.sdfk_volume_integrate_depth(None, None, A, 4, 4, cam, m, C.byref(prm), st),
        "sdfk_volume_integrate_depth_device": lambda: L.sdfk_volume_integrate_depth_device(None, None, A, 4, 4, cam, m, C.byref(prm), st),
        "sdfk_depth_unproject": lambda: L.sdfk_depth_unproject(A, None, 4, 4, cam, m, 1.0, 100.0, None, None, None, C.byref(n)),
        "sdfk_depth_unproject_device": lambda: L.sdfk_depth_unproject_device(A, None, 4, 4, cam, m, 1.0, 100.0, None, None, None, C.byref(n)),
    }
    assert sorted(calls) == sorted(ENTRY_POINTS)
    for name, call in calls.items():
        assert call() == N.ERR_NO_DEVICE, name
    assert n.value == -7 and list(st) == [-7] * 4


# ---- accuracy, through the model ----
SETUPS = {"sphere_32_64px_14_views_carved": ("sphere", 32, 64, range(14), True),
          "sphere_48_128px_14_views_carved": ("sphere", 48, 128, range(14), True),
          "two_spheres_32_64px_14_views_carved": ("two_spheres", 32, 64, range(14), True),
          "sphere_32_64px_6_views_open": ("sphere", 32, 64, range(6), False)}


def accuracy_figures():
    return {name: M.accuracy(*args, Cs.camera) for name, args in SETUPS.items()}


def test_recorded_accuracy_is_reproduced_and_a_closed_scan_is_within_a_voxel():
    """Analytic ray depth of the library's own camera arithmetic, 14 views at distance 4 to 4.3 around the box -+1.5, truncation three
    voxels, weight 1 (6 views for the open variant).  Carved closed scans: no voxel beyond one voxel of the surface has the wrong
    sign, and every zero crossing on a grid edge lies within one voxel of the surface (recorded: 0.51 to 0.55 at most, 0.12 to 0.14
    in the mean).  The open variant is recorded only: its sheet one truncation behind the surface is what the unseen convention
    describes."""
    fig = accuracy_figures()
    for name, f in fig.items():
        print(name, f)
    with open(GOLDEN) as f:
        assert json.load(f) == fig
    for name, f in fig.items():
        if name.endswith("carved"):
            assert f["wrong_signs_beyond_one_voxel"] == 0 and f["crossing_error_max_voxels"] < 1.0 and f["crossings"] > 500, name
    assert fig["sphere_32_64px_6_views_open"]["wrong_signs_beyond_one_voxel"] > 1000
    # the occlusion of the two-sphere scene is real: from +x the small sphere hides part of the large one
    pos, _, vpi, _, _ = Cs.camera(64, 64, M.view(0))
    both = M.sphere_depth(64, 64, pos, vpi, M.SCENES["two_spheres"])
    far_one = M.sphere_depth(64, 64, pos, vpi, M.SCENES["two_spheres"][:1])
    assert (np.isfinite(far_one) & (both < far_one)).sum() > 50


def test_unprojected_points_are_the_renders_hit_points():
    """A frame rendered by the model of sdfk_trimesh_render (tests/mesh_ray_model.py): DepthToPoints' arithmetic gives that render's
    camera + r * distance at every pixel that hit, bit for bit, in pixel order."""
    from tests import mesh_ray_cases as RC
    from tests import mesh_ray_model as RM
    for name in ("cube_2x2", "inside_sphere", "sphere_64x48"):
        c = RC.render_case(name)
        depth, _, tri = RC.render_model(name)
        pts, _, pix = M.unproject(depth, c["cam"], c["vpi"], c["near"], c["far"])
        hit = np.flatnonzero(tri.reshape(-1) >= 0)
        assert np.array_equal(pix, hit), name
        R = RM.camera_rays(c["width"], c["height"], c["cam"], c["vpi"])[hit]
        cam = np.asarray(c["cam"], f32)
        want = np.stack([(cam[a] + (R[:, a] * depth.reshape(-1)[hit]).astype(f32)).astype(f32) for a in range(3)], -1)
        assert Cs.bits_equal(pts, want.reshape(-1, 3)), name
    assert len(hit) > 0
