"""Depth fusion and unprojection on the device (sdfk_volume_integrate_depth / sdfk_depth_unproject, csrc/lib_fusion.hip) against the
numpy model (tests/depth_fusion_model.py) bit for bit: every case of tests/depth_fusion_cases.py through the host form, the _device
form and the Python layer (DepthFusion, DepthToPoints) -- values, weights, stats, points, colours, pixels; the refusals through the
C ABI, with nothing written; and end to end on the device alone: a closed mesh rendered from 14 poses, fused, redistanced and meshed
is watertight and within one voxel of the scanned mesh, and a frame's points register onto samples of the mesh."""
import ctypes as C

import numpy as np
import pytest

from sdfkit_amd import DepthFusion, DepthToPoints, IterativeClosestPoint, KdTree, SdfFuncs
from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import MeshSdf
from tests import depth_fusion_cases as Cs
from tests import depth_fusion_model as M

pytestmark = pytest.mark.gpu

f32, f64, u32, i32 = np.float32, np.float64, np.uint32, np.int32


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p()


def _m16(m):
    return (C.c_float * 16)(*[float(x) for x in np.asarray(m, f32).ravel()])


class Vol:
    """A raw sdfk_volume (whole or slab) holding `values`"""

    def __init__(self, values, mn, mx, z0=0, nz_global=None):
        nx, ny, nz = values.shape
        self.shape = values.shape
        self.h = C.c_void_p()
        N.check(N.lib().sdfk_volume_create_slab(nx, ny, nz if nz_global is None else nz_global, N.f3(mn), N.f3(mx), z0, nz, 0, C.byref(self.h)))
        self.upload(values)

    def upload(self, values):
        N.check(N.lib().sdfk_volume_upload(self.h, _vp(np.ascontiguousarray(values, f32)), None))

    def download(self):
        out = np.empty(self.shape, f32)
        N.check(N.lib().sdfk_volume_download(self.h, _vp(out), None))
        return out

    def free(self):
        if self.h:
            N.lib().sdfk_volume_free(self.h)
        self.h = None


def _params(c, fr):
    return N.FusionParams(float(c["truncation"]), float(fr["depth_min"]), float(fr["depth_max"]), float(fr["weight"]), float(c["max_weight"]),
                          int(fr["flags"]))


def _integrate_raw(name, device):
    c = Cs.volume_case(name)
    D, W = (Vol(c[k], c["mn"], c["mx"], c["z0"], c["nz_global"]) for k in ("D0", "W0"))
    stats = []
    try:
        for fr in c["frames"]:
            h, w = fr["depth"].shape
            st = (C.c_int64 * 4)(-7, -7, -7, -7)
            prm = _params(c, fr)
            if device:
                import torch
                dd = torch.from_numpy(fr["depth"]).to(torch.device("cuda", N.init()))
                torch.cuda.synchronize()
                N.check(N.lib().sdfk_volume_integrate_depth_device(D.h, W.h, C.c_void_p(dd.data_ptr()), w, h, N.f3(fr["pos"]), _m16(fr["vp"]),
                                                                   C.byref(prm), st))
                N.check(N.lib().sdfk_synchronize())
            else:
                N.check(N.lib().sdfk_volume_integrate_depth(D.h, W.h, _vp(fr["depth"]), w, h, N.f3(fr["pos"]), _m16(fr["vp"]), C.byref(prm), st))
            stats.append(list(st))
        return D.download(), W.download(), stats
    finally:
        D.free()
        W.free()


@pytest.mark.parametrize("name", list(Cs.VOLUMES))
def test_integrate_host_form_equals_model(gpu, name):
    D, W, stats = Cs.volume_model(name)
    gD, gW, gstats = _integrate_raw(name, False)
    assert gstats == stats
    assert Cs.bits_equal(gD, D), np.argwhere(gD.view(u32) != D.view(u32))[:8]
    assert Cs.bits_equal(gW, W), np.argwhere(gW.view(u32) != W.view(u32))[:8]
    if name in Cs.NOTHING_WRITTEN:
        c = Cs.volume_case(name)
        assert gstats[0][0] == 0 and Cs.bits_equal(gD, c["D0"]) and Cs.bits_equal(gW, c["W0"])


@pytest.mark.parametrize("name", ["sphere_5x6x7_carve", "sphere_3x2x9_open", "sphere_2x3x261_carve", "sphere_33x17x12_open", "slab", "image_1x1_all",
                                  "exact_axis", "frustum_misses", "odd_depths_carve", "sequence_max_weight", "seeded_weights"])
def test_integrate_device_form_equals_model(gpu, name):
    D, W, stats = Cs.volume_model(name)
    gD, gW, gstats = _integrate_raw(name, True)
    assert gstats == stats and Cs.bits_equal(gD, D) and Cs.bits_equal(gW, W)


def test_slab_equals_the_planes_of_the_whole_volume(gpu):
    D, W, _ = _integrate_raw("slab", False)
    Dw, Ww, _ = _integrate_raw("slab_whole", False)
    assert Cs.bits_equal(D, Dw[:, :, 3:8]) and Cs.bits_equal(W, Ww[:, :, 3:8])


def test_stats_may_be_null(gpu):
    name = "sphere_5x6x7_carve"
    c = Cs.volume_case(name)
    fr = c["frames"][0]
    D, W = (Vol(c[k], c["mn"], c["mx"]) for k in ("D0", "W0"))
    try:
        h, w = fr["depth"].shape
        prm = _params(c, fr)
        N.check(N.lib().sdfk_volume_integrate_depth(D.h, W.h, _vp(fr["depth"]), w, h, N.f3(fr["pos"]), _m16(fr["vp"]), C.byref(prm), None))
        assert Cs.bits_equal(D.download(), Cs.volume_model(name)[0]) and Cs.bits_equal(W.download(), Cs.volume_model(name)[1])
    finally:
        D.free()
        W.free()


@pytest.mark.parametrize("name", ["sphere_5x6x7_carve", "sphere_2x3x261_open", "image_2x2_alternating", "camera_inside", "camera_at_cell_centre",
                                  "exact_axis", "odd_depths_open", "sequence", "sequence_weight_half", "seeded_weights"])
def test_depth_fusion_class_equals_model(gpu, name):
    c = Cs.volume_case(name)
    D, W, stats = Cs.volume_model(name)
    carve = bool(c["frames"][0]["flags"])
    fu = DepthFusion(c["mn"], c["mx"], *c["shape"], float(c["truncation"]), unseen=float(c["D0"].flat[0]), carve=carve,
                     maxWeight=float(c["max_weight"]))
    assert np.all(fu.Weights.Values == 0) and np.all(fu.Values.Values == c["D0"].flat[0])
    if name == "seeded_weights":   # host arrays the caller edits win, as for every Voxels
        fu.Values.Values[...] = c["D0"]
        fu.Weights.Values[...] = c["W0"]
    for fr, want in zip(c["frames"], stats):
        st = {}
        fu.Integrate(fr["depth"], *fr["cam"], weight=float(fr["weight"]), depthMin=float(fr["depth_min"]), depthMax=float(fr["depth_max"]),
                     stats=st, **fr["lens"])
        assert [st["updated"], st["surface"], st["first"], st["valid_pixels"]] == want
    assert fu.Frames == len(c["frames"]) and fu.ToVoxels() is fu.Values
    assert Cs.bits_equal(fu.Values.Values, D) and Cs.bits_equal(fu.Weights.Values, W)


def test_integrate_device_through_the_class(gpu):
    import torch
    name = "sphere_33x17x12_carve"
    c = Cs.volume_case(name)
    fr = c["frames"][0]
    fu = DepthFusion(c["mn"], c["mx"], *c["shape"], float(c["truncation"]))
    dd = torch.from_numpy(fr["depth"]).to(torch.device("cuda", N.init()))
    torch.cuda.synchronize()
    st = {}
    h, w = fr["depth"].shape
    fu.IntegrateDevice(dd.data_ptr(), w, h, fr["pos"], fr["vp"], float(fr["depth_min"]), float(fr["depth_max"]), stats=st)
    D, W, stats = Cs.volume_model(name)
    assert [st["updated"], st["surface"], st["first"], st["valid_pixels"]] == stats[0]
    assert Cs.bits_equal(fu.Values.Values, D) and Cs.bits_equal(fu.Weights.Values, W)


# ---- unprojection -------------------------------------------------------------------------------------------------------------------
def _unproject_raw(c, device, want_points=True, want_colors=True, want_pixel=True):
    n = c["width"] * c["height"]
    rgb = c["rgb"]
    want_colors = want_colors and rgb is not None
    k = C.c_int64(-7)
    args = (c["width"], c["height"], N.f3(c["pos"]), _m16(c["vpi"]), C.c_float(c["depth_min"]), C.c_float(c["depth_max"]))
    if device:
        import torch
        dev = torch.device("cuda", N.init())
        dd = torch.from_numpy(c["depth"]).to(dev)
        cc = torch.from_numpy(rgb).to(dev) if rgb is not None else None
        pts = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device=dev)
        cols = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device=dev)
        pix = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        r = N.lib().sdfk_depth_unproject_device(C.c_void_p(dd.data_ptr()), C.c_void_p(cc.data_ptr()) if cc is not None else None, *args,
                                                C.c_void_p(pts.data_ptr()) if want_points else None,
                                                C.c_void_p(cols.data_ptr()) if want_colors else None,
                                                C.c_void_p(pix.data_ptr()) if want_pixel else None, C.byref(k))
        N.check(N.lib().sdfk_synchronize())
        pts, cols, pix = pts.cpu().numpy(), cols.cpu().numpy(), pix.cpu().numpy()
        m = max(k.value, 0)
        assert np.all(pts[m:] == -7) and np.all(cols[m:] == -7) and np.all(pix[m:] == -7)   # the device form writes n_valid entries
    else:
        pts, cols, pix = np.full((n + 1, 3), -7, f32), np.full((n + 1, 3), -7, f32), np.full(n + 1, -7, i32)
        r = N.lib().sdfk_depth_unproject(_vp(c["depth"]), _vp(rgb), *args, _vp(pts) if want_points else None, _vp(cols) if want_colors else None,
                                         _vp(pix) if want_pixel else None, C.byref(k))
        assert np.all(pts[n:] == -7) and np.all(cols[n:] == -7) and np.all(pix[n:] == -7)   # nothing past the arrays' end
    m = k.value
    return r, m, pts[:m] if want_points else None, cols[:m] if want_colors else None, pix[:m] if want_pixel else None


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(Cs.FRAMES))
def test_unproject_equals_model(gpu, name, device):
    c = Cs.frame_case(name)
    pts, cols, pix = Cs.frame_model(name)
    r, n, gp, gc, gx = _unproject_raw(c, device)
    assert r == 0 and n == len(pix)
    assert np.array_equal(gx, pix) and Cs.same_f32(gp, pts)
    assert (cols is None and gc is None) or Cs.bits_equal(gc, cols)


def test_unproject_null_outputs(gpu):
    c = Cs.frame_case("3x5_alternating")
    pts, cols, pix = Cs.frame_model("3x5_alternating")
    for sel in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        for device in (False, True):
            r, n, gp, gc, gx = _unproject_raw(c, device, *sel)
            assert r == 0 and n == len(pix)
            assert (gp is None or Cs.same_f32(gp, pts)) and (gc is None or Cs.bits_equal(gc, cols)) and (gx is None or np.array_equal(gx, pix))


@pytest.mark.parametrize("name", ["scene_64x48", "scene_no_rgb", "2x2_alternating", "241x272_alternating"])
def test_depth_to_points_equals_model(gpu, name):
    c = Cs.frame_case(name)
    pts, cols, pix = Cs.frame_model(name)
    gp, gc, gx = DepthToPoints(c["depth"], *c["cam"], rgb=c["rgb"])
    assert np.array_equal(gx, pix) and Cs.same_f32(gp, pts) and ((cols is None and gc is None) or Cs.bits_equal(gc, cols))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_integrate_refusals_write_nothing(gpu):
    L = N.lib()
    rng = np.random.default_rng(0)
    made = {}

    def vol(v):
        key = (v["shape"], v["nz_global"], v["z0"], v["mn"], v["mx"])
        if key not in made:
            made[key] = []
        data = rng.uniform(-1, 1, v["shape"]).astype(f32)
        made[key].append((Vol(data, v["mn"], v["mx"], v["z0"], v["nz_global"]), data))
        return made[key][-1]

    depth = np.full((3, 4), 2.0, f32)
    cam, m = N.f3((0, 0, 3)), _m16(Cs.camera(4, 3, ((0, 0, 3), (0, 0, 0), (0, 1, 0)))[1])
    try:
        for who in (L.sdfk_volume_integrate_depth, L.sdfk_volume_integrate_depth_device):
            for name, (changes, word) in Cs.REFUSALS.items():
                if name == "no_storage":   # (no entry point hands out a volume without storage)
                    continue
                c = dict(Cs.GOOD, **changes)
                (a, da), (b, db) = vol(c["a"]), vol(c["b"])
                prm = N.FusionParams(c["truncation"], c["depth_min"], c["depth_max"], c["weight"], c["max_weight"], c["flags"])
                st = (C.c_int64 * 4)(-7, -7, -7, -7)
                assert who(a.h, b.h, _vp(depth), c["width"], c["height"], cam, m, C.byref(prm), st) == N.ERR_INVALID, name
                msg = L.sdfk_last_error().decode()
                assert "sdfk_volume_integrate_depth" in msg and word in msg, (name, msg)
                assert list(st) == [-7] * 4 and Cs.bits_equal(a.download(), da) and Cs.bits_equal(b.download(), db), name
            (a, da), (b, db) = vol(Cs.GOOD["a"]), vol(Cs.GOOD["b"])
            prm = N.FusionParams(0.25, 1.0, 100.0, 1.0, np.inf, 1)
            good = [a.h, b.h, _vp(depth), 4, 3, cam, m, C.byref(prm), None]
            for k, word in ((0, "null"), (1, "null"), (2, "null"), (5, "null"), (6, "null"), (7, "null")):
                args = list(good)
                args[k] = None
                assert who(*args) == N.ERR_INVALID and word in L.sdfk_last_error().decode(), k
            assert who(a.h, a.h, *good[2:]) == N.ERR_INVALID and "same volume" in L.sdfk_last_error().decode()
            assert Cs.bits_equal(a.download(), da) and Cs.bits_equal(b.download(), db)
        # ... and the good call is accepted, with every accepted edge of the table
        for name, changes in Cs.ACCEPTED.items():
            if name == "huge_image":
                continue
            c = dict(Cs.GOOD, **changes)
            (a, _), (b, _) = vol(c["a"]), vol(c["b"])
            prm = N.FusionParams(c["truncation"], c["depth_min"], c["depth_max"], c["weight"], c["max_weight"], c["flags"])
            assert L.sdfk_volume_integrate_depth(a.h, b.h, _vp(depth), c["width"], c["height"], cam, m, C.byref(prm), None) == 0, name
    finally:
        for vols in made.values():
            for v, _ in vols:
                v.free()


def test_unproject_refusals_write_nothing(gpu):
    L = N.lib()
    depth, rgb = np.full((3, 4), 2.0, f32), np.ones((3, 4, 3), f32)
    pos, _, vpi, _, _ = Cs.camera(4, 3, ((0, 0, 3), (0, 0, 0), (0, 1, 0)))
    cam, m = N.f3(pos), _m16(vpi)
    pts, cols, pix = np.full((12, 3), -7, f32), np.full((12, 3), -7, f32), np.full(12, -7, i32)
    k = C.c_int64(-7)
    good = [_vp(depth), _vp(rgb), 4, 3, cam, m, C.c_float(1.0), C.c_float(100.0), _vp(pts), _vp(cols), _vp(pix), C.byref(k)]
    bad = [({0: None}, "null"), ({4: None}, "null"), ({5: None}, "null"), ({11: None}, "null"), ({1: None}, "colors3"), ({2: 0}, "width"),
           ({3: -1}, "height"), ({2: 1 << 16, 3: 1 << 15}, "2^31"), ({6: C.c_float(np.nan)}, "NaN"), ({7: C.c_float(np.nan)}, "NaN"),
           ({6: C.c_float(3.0), 7: C.c_float(2.0)}, "depth_min")]
    for who in (L.sdfk_depth_unproject, L.sdfk_depth_unproject_device):   # (refused before any pointer is used: host arrays serve both)
        for changes, word in bad:
            args = list(good)
            for i, v in changes.items():
                args[i] = v
            assert who(*args) == N.ERR_INVALID, changes
            msg = L.sdfk_last_error().decode()
            assert "sdfk_depth_unproject" in msg and word in msg, (changes, msg)
        assert k.value == -7 and np.all(pts == -7) and np.all(cols == -7) and np.all(pix == -7)
    assert L.sdfk_depth_unproject(*good) == 0 and k.value == 12


# ---- end to end, on the device alone --------------------------------------------------------------------------------------------------
def test_scan_of_a_closed_mesh_is_watertight_and_within_a_voxel(gpu):
    """A union of two spheres, meshed at 48^3, is rendered by MeshSdf.RenderDepth from the 14 poses of the accuracy set-up (128^2
    pixels: a pixel is 0.036 wide at the object, half a voxel), fused into 40^3 voxels of 0.075 with a truncation of three voxels,
    redistanced and meshed.  The result is watertight, and every vertex lies within one voxel of the scanned mesh -- the first-order
    bound the model's closed scans meet with 0.55 voxels at most (tests/golden/depth_fusion_accuracy.json).  A frame's points lie on
    the scanned mesh, and from a pose that is off by 0.04 they register onto samples of the mesh nearer than they began."""
    mn, mx, n = [-1.5] * 3, [1.5] * 3, 40
    voxel = 3.0 / n
    scene = SdfFuncs.Union(SdfFuncs.Sphere(0.8).Translate(-0.3, 0.0, 0.0), SdfFuncs.Sphere(0.55).Translate(0.6, 0.2, 0.1)).ToSdf()
    mesh = scene.ToMesh(mn, mx, 48, 48, 48)
    scanned = MeshSdf(mesh)
    assert scanned.Topology().IsWatertight
    fu = DepthFusion(mn, mx, n, n, n, 3 * voxel)
    frames = []
    for k in range(14):
        view = M.view(k)
        frames.append(scanned.RenderDepth(128, 128, *view))
        st = {}
        fu.Integrate(frames[-1], *view, stats=st)
        assert st["surface"] > 100 and st["updated"] > st["surface"] and st["valid_pixels"] == int(np.isfinite(frames[-1].Values).sum())
    fused = fu.ToMesh()
    top = fused.Topology()
    assert top.IsWatertight and top.Triangles > 1000 and top.BoundaryEdges == 0
    _, dist, _ = scanned.Search(fused.Vertices)
    print(f"fused mesh: {top.Triangles} triangles, vertex distance to the scanned mesh max {dist.max() / voxel:.3f} mean {dist.mean() / voxel:.3f} voxels")
    assert dist.max() < voxel
    # a frame as points: on the mesh, and registering onto samples of it
    pts, _, pix = DepthToPoints(frames[0], *M.view(0))
    assert len(pts) == int(np.isfinite(frames[0].Values).sum()) > 1000
    _, on, _ = scanned.Search(pts)
    assert on.max() < 1e-5
    static = scanned.SamplePoints(30000, seed=1).Points
    tree = KdTree(pts)   # the frame as a search structure: the visible samples of the mesh have a scanned point within two pixels
    _, near, _ = tree.SearchMany(static)
    assert tree.TotalPoints == len(pts) and (near < 2 * 0.036).sum() > len(static) // 8
    moved = np.ascontiguousarray(pts + np.array([0.03, -0.02, 0.015], f32), f32)
    before = float(np.linalg.norm(moved.astype(f64) - pts, axis=1).mean())
    icp = IterativeClosestPoint(static)
    icp.GoodCorrespondenceDistance = f32(0.2)
    icp.RegisterPoints(moved)
    after = float(np.linalg.norm(moved.astype(f64) - pts, axis=1).mean())
    print(f"registration: mean offset {before:.4f} -> {after:.4f} in {icp.Iterations} iterations")
    assert after < before
