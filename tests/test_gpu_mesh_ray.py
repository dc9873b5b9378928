"""Rays against triangle meshes on the device (sdfk_trimesh_raycast / sdfk_trimesh_render, csrc/lib_trimesh_ray.hip) through the
Python layers, against the numpy model (tests/mesh_ray_model.py: brute force over all triangles) bit for bit: every case of
tests/mesh_ray_cases.py, host and device forms, the any-hit flag, NULL outputs in every combination, the renders; the diagnostic
counts against the host program's (tests/cpp/mesh_ray_host.cpp runs the same walk: equal counts mean the device ran it too); the
refusals; and the properties: Occluded == Hit, the hit point from the weights, even crossings of closed meshes, the accuracy on a
marching-cubes sphere, the sky of a render against the ray marcher's."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from sdfkit_amd import Mesh, Sdfs
from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import RAY_ANY_HIT, MeshSdf
from sdfkit_amd.raymarch import Matrix4x4, RayMarcher
from tests import mesh_ray_cases as Cs
from tests import mesh_ray_model as M

pytestmark = pytest.mark.gpu

f32, f64, u32, i32 = np.float32, np.float64, np.uint32, np.int32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_ray_accuracy.json")


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_ray_gpu")
    return Cs.build_host(d), d


@pytest.fixture(scope="module")
def handle(gpu):
    """handle(case) -> one MeshSdf per mesh of the cases (several cases share a mesh); all are freed when the module is done"""
    made = {}

    def get(c):
        key = (c["V"].tobytes(), c["T"].tobytes(), None if c.get("colors") is None else c["colors"].tobytes())
        if key not in made:
            made[key] = MeshSdf((c["V"], c["T"]) if c.get("colors") is None else (c["V"], c["T"], c["colors"]))
        return made[key]

    yield get
    for t in made.values():
        t.__del__()   # (sdfk_trimesh_free now, not at collection)
    made.clear()


def raw_cast(t, c, flags, want_tri=True, want_dist=True, want_w=True):
    """sdfk_trimesh_raycast with any subset of the outputs -> (status, triangle, distance, weights)"""
    n = len(c["O"])
    tri = np.full(n + 1, -7, i32) if want_tri else None
    dist = np.full(n + 1, -7, f32) if want_dist else None
    w = np.full((n + 1, 3), -7, f32) if want_w else None
    r = N.lib().sdfk_trimesh_raycast(t.handle, _vp(c["O"]) if n else None, _vp(c["D"]) if n else None, n, C.c_float(c["tmin"]), C.c_float(c["tmax"]),
                                     flags, _vp(tri), _vp(dist), _vp(w))
    for a in (tri, dist, w):
        assert a is None or np.all(a[n:] == -7)   # nothing past the end
    return r, None if tri is None else tri[:n], None if dist is None else dist[:n], None if w is None else w[:n]


# ---- every case, host form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.CASES))
def test_raycast_equals_model_bit_for_bit(gpu, handle, name):
    c, want = Cs.case(name), Cs.model(name)
    t = handle(c)
    hits = t.RayCast(c["O"], c["D"], c["tmin"], c["tmax"])
    assert np.array_equal(hits.Triangles, want.triangle), np.flatnonzero(hits.Triangles != want.triangle)[:8]
    assert np.array_equal(bits(hits.Distances), bits(want.distance)) and np.array_equal(bits(hits.Weights), bits(want.weights))
    assert np.array_equal(hits.Hit, want.triangle >= 0)
    # the any-hit flag, and Occluded == Hit
    r, tri, _, _ = raw_cast(t, c, RAY_ANY_HIT, True, False, False)
    assert r == 0 and np.array_equal(tri, np.where(want.triangle >= 0, 0, -1))
    assert np.array_equal(tri, Cs.model(name, M.ANY_HIT).triangle)
    assert np.array_equal(t.Occluded(c["O"], c["D"], c["tmin"], c["tmax"]), hits.Hit)


@pytest.mark.parametrize("name", ["cube", "bad_rays", "count_257"])
def test_null_outputs_in_every_combination(gpu, handle, name):
    c, want = Cs.case(name), Cs.model(name)
    t = handle(c)
    for wt, wd, ww in itertools.product((False, True), repeat=3):
        r, tri, dist, w = raw_cast(t, c, 0, wt, wd, ww)
        assert r == 0
        assert tri is None or np.array_equal(tri, want.triangle)
        assert dist is None or np.array_equal(bits(dist), bits(want.distance))
        assert w is None or np.array_equal(bits(w), bits(want.weights))
    for wt in (False, True):
        r, tri, _, _ = raw_cast(t, c, RAY_ANY_HIT, wt, False, False)
        assert r == 0 and (tri is None or np.array_equal(tri >= 0, want.triangle >= 0))


# ---- hit points from the weights -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "sphere", "walk_traps", "far_mesh", "flat_mesh", "scale_1e30"])
def test_hit_point_from_weights_agrees_with_the_ray(gpu, handle, name):
    """P_w = wa a + wb b + wc c and P_r = o + t d, both in float64 from the f32 outputs, are one point up to the roundings of the
    outputs: each weight is within 2^-24 |w| of its binary64 value, so P_w moves by at most 2^-24 (|wa a| + |wb b| + |wc c|) per
    component; t is within 2^-24 |t|, so P_r moves by at most 2^-24 |t d|.  The binary64 arithmetic before the rounding adds its
    own error, relative 2^-52 amplified by the conditioning of the quotients (grazing rays): 2^-36 of the magnitudes involved
    allows an amplification of 2^16."""
    c = Cs.case(name)
    hits = handle(c).RayCast(c["O"], c["D"], c["tmin"], c["tmax"])
    h = hits.Hit
    assert h.any()
    V, T = c["V"].astype(f64), c["T"][hits.Triangles[h]]
    w = hits.Weights[h].astype(f64)
    terms = [w[:, k, None] * V[T[:, k]] for k in range(3)]
    Pw = terms[0] + terms[1] + terms[2]
    td = hits.Distances[h].astype(f64)[:, None] * c["D"][h].astype(f64)
    Pr = c["O"][h].astype(f64) + td
    mag = sum(np.abs(x) for x in terms)
    bound = 2.0 ** -24 * (mag + np.abs(td)) + 2.0 ** -36 * (mag + np.abs(td) + np.abs(c["O"][h].astype(f64)))
    err = np.abs(Pw - Pr)
    print(f"{name}: max error / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    assert np.array_equal(bits(hits.Points()), bits((c["O"][h] + c["D"][h] * hits.Distances[h, None]).astype(f32)))


# ---- closed meshes: an even number of sheets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Cs.CLOSED)
def test_rays_from_outside_cross_closed_meshes_an_even_number_of_times(gpu, handle, name):
    """The sheets are counted by casting again from just beyond each hit (tMin = the next f32 after its distance).  The rays are
    the case's RANDOM rays from outside.  Its aimed ones pass through vertices and edge midpoints, those of the silhouette
    included, where the ray touches the surface: two sheets at one t, which this way of counting cannot tell apart (on the CPU,
    with the host program, exactly such rays count 1)."""
    c = Cs.case(name)
    t = handle(c)
    n = len(c["O"])
    pick = np.arange(n - Cs.OUTSIDE_RANDOM[name], n)[::Cs.OUTSIDE_RANDOM[name] // 64]
    crossed = []
    for r in pick:
        tmin, k = f32(0.0), 0
        while True:
            hit = t.RayCast(c["O"][r], c["D"][r], tmin, np.inf)
            if not hit.Hit[0]:
                break
            k += 1
            assert k < 64
            tmin = np.nextafter(hit.Distances[0], f32(np.inf))   # just beyond this sheet
        crossed.append(k)
    crossed = np.array(crossed)
    assert np.all(crossed % 2 == 0), (pick[crossed % 2 == 1], crossed)
    assert (crossed > 0).any() and (crossed == 0).any()


# ---- the diagnostic counts: the device ran the host program's walk ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.CASES))
def test_profiled_counts_equal_the_host_walk(gpu, handle, host, name):
    exe, d = host
    c = Cs.case(name)
    t = handle(c)
    head, tri, *_ = Cs.host_cast(exe, d, c)
    s0 = t.stats()
    assert tuple(s0["grid"]) == head["dim"] and s0["entries"] == head["entries"]      # the grid the host program rebuilt is the handle's
    N.check(N.lib().sdfk_profile_enable(1))
    try:
        hits = t.RayCast(c["O"], c["D"], c["tmin"], c["tmax"])
        s = t.stats()
        if len(c["O"]) == 0:   # n == 0 touches nothing, the counts of the last query included
            assert (s["candidates"], s["queries"]) == (s0["candidates"], s0["queries"]) and head["tests"] == 0
            return
        assert (s["candidates"], s["queries"]) == (head["tests"], head["n"]) == (head["tests"], len(c["O"]))
        assert np.array_equal(hits.Triangles, tri)
        if name == "sphere_inside_random":
            # a condition, not a measurement: brute force must not pass as a walk (met by the host program first: test_mesh_ray_host.py)
            assert head["tests"] < head["n"] * len(c["T"]) / 10
            assert s["candidates"] < s["queries"] * len(c["T"]) / 10
        # any hit: the same rays, and no more tests than the first-hit walk (the order inside a cell decides where it stops)
        t.Occluded(c["O"], c["D"], c["tmin"], c["tmax"])
        sa = t.stats()
        assert sa["queries"] == len(c["O"]) and sa["candidates"] <= s["candidates"]
    finally:
        N.check(N.lib().sdfk_profile_enable(0))


@pytest.mark.parametrize("name", list(Cs.RENDER))
def test_profiled_counts_of_a_render(gpu, handle, host, name):
    exe, d = host
    c = Cs.render_case(name)
    t = handle(c)
    head, *_ = Cs.host_render(exe, d, c)
    N.check(N.lib().sdfk_profile_enable(1))
    try:
        depth, rgb = np.empty((c["height"], c["width"]), f32), np.empty((c["height"], c["width"], 3), f32)
        for images in ((depth, None), (None, rgb)):   # the images asked for do not change the walk
            N.check(N.lib().sdfk_trimesh_render(t.handle, c["width"], c["height"], N.f3(c["cam"]), (C.c_float * 16)(*[float(x) for x in c["vpi"].ravel()]),
                                                C.c_float(c["near"]), C.c_float(c["far"]), _vp(images[0]), _vp(images[1]), None))
            s = t.stats()
            assert (s["candidates"], s["queries"]) == (head["tests"], c["width"] * c["height"])
    finally:
        N.check(N.lib().sdfk_profile_enable(0))


# ---- the device forms ----------------------------------------------------------------------------------------------------------------
def _meshed_sphere_handle():
    """a handle made by sdfk_trimesh_create_device straight from the device arrays of a meshed sphere: no host round trip"""
    L = N.lib()
    m = C.c_void_p()
    n = 32
    sdf = Sdfs.Sphere(1.0)   # (held: the program handle dies with the Sdf object)
    N.check(L.sdfk_sample_march(sdf.program(), N.f3([-1.25] * 3), N.f3([1.25] * 3), n, n, n, 0, C.c_float(0.0), 1, C.byref(m)))
    try:
        nv, ni = C.c_int64(), C.c_int64()
        N.check(L.sdfk_mesh_counts(m, C.byref(nv), C.byref(ni)))
        vp, tp = C.c_void_p(), C.c_void_p()
        N.check(L.sdfk_mesh_device_ptrs(m, C.byref(vp), None, None, C.byref(tp)))
        h = C.c_void_p()
        N.check(L.sdfk_trimesh_create_device(vp, nv.value, tp, ni.value, None, C.byref(h)))
        V, T = np.empty((nv.value, 3), f32), np.empty(ni.value, i32)
        N.check(L.sdfk_mesh_copy(m, _vp(V), None, None, _vp(T)))   # (for the comparison only)
    finally:
        L.sdfk_mesh_free(m)
    t = MeshSdf.__new__(MeshSdf)
    t._h, t.Colors, t.Vertices, t.Triangles = h, None, V, T
    return t


def test_device_forms_on_a_device_made_handle(gpu):
    import torch
    t = _meshed_sphere_handle()
    c = Cs.case("sphere")
    assert np.array_equal(bits(t.Vertices), bits(c["V"])) and np.array_equal(t.Triangles.reshape(-1, 3), c["T"])   # the case's mesh: its model serves
    want = Cs.model("sphere")
    dev = torch.device("cuda", N.init())
    n = len(c["O"])
    o, d = torch.from_numpy(c["O"]).to(dev), torch.from_numpy(c["D"]).to(dev)
    tri = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((n + 1,), -7.0, dtype=torch.float32, device=dev)
    w = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device=dev)
    occ = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t.RayCastDevice(o.data_ptr(), d.data_ptr(), n, c["tmin"], c["tmax"], tri.data_ptr(), dist.data_ptr(), w.data_ptr())
    t.RayCastDevice(o.data_ptr(), d.data_ptr(), n, c["tmin"], c["tmax"], occ.data_ptr(), None, None, anyHit=True)
    N.check(N.lib().sdfk_synchronize())
    tri, dist, w, occ = tri.cpu().numpy(), dist.cpu().numpy(), w.cpu().numpy(), occ.cpu().numpy()
    assert tri[-1] == -7 and dist[-1] == -7 and np.all(w[-1] == -7) and occ[-1] == -7
    assert np.array_equal(tri[:-1], want.triangle) and np.array_equal(bits(dist[:-1]), bits(want.distance))
    assert np.array_equal(bits(w[:-1]), bits(want.weights)) and np.array_equal(occ[:-1] >= 0, want.triangle >= 0)
    # render_device: the three images, and each alone
    rc = Cs.render_case("sphere_64x48")
    wd, wrgb, wtri = Cs.render_model("sphere_64x48")
    px = rc["width"] * rc["height"]
    for sel in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        dd = torch.full((px + 1,), -7.0, dtype=torch.float32, device=dev)
        cc = torch.full((px + 1, 3), -7.0, dtype=torch.float32, device=dev)
        tt = torch.full((px + 1,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t.RenderDevice(rc["width"], rc["height"], rc["cam"], rc["vpi"], rc["near"], rc["far"], dd.data_ptr() if sel[0] else None,
                       cc.data_ptr() if sel[1] else None, tt.data_ptr() if sel[2] else None)
        N.check(N.lib().sdfk_synchronize())
        dd, cc, tt = dd.cpu().numpy(), cc.cpu().numpy(), tt.cpu().numpy()
        assert np.array_equal(bits(dd[:-1]), bits(wd.reshape(-1))) if sel[0] else np.all(dd == -7)
        assert np.array_equal(bits(cc[:-1]), bits(wrgb.reshape(-1, 3))) if sel[1] else np.all(cc == -7)
        assert np.array_equal(tt[:-1], wtri.reshape(-1)) if sel[2] else np.all(tt == -7)
        assert dd[-1] == -7 and np.all(cc[-1] == -7) and tt[-1] == -7


# ---- renders ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.RENDER))
def test_render_equals_model_bit_for_bit(gpu, handle, name):
    c = Cs.render_case(name)
    depth, rgb, tri = Cs.render_model(name)
    t = handle(c)
    lens = dict(nearPlaneDistance=c["near"], farPlaneDistance=c["far"])
    assert np.array_equal(bits(t.RenderDepth(c["width"], c["height"], *c["camera"], **lens).Values), bits(depth))
    assert np.array_equal(bits(t.Render(c["width"], c["height"], *c["camera"], **lens).Values), bits(rgb))
    assert np.array_equal(t.RenderTriangles(c["width"], c["height"], *c["camera"], **lens), tri)
    # all three images of one call
    d3, c3, t3 = t._render(c["width"], c["height"], c["camera"], lens, True, True, True)
    assert np.array_equal(bits(d3), bits(depth)) and np.array_equal(bits(c3), bits(rgb)) and np.array_equal(t3, tri)
    # Mesh.ToImage: the signature of SdfEx.ToImage
    mesh = Mesh(c["V"], c["colors"], None, c["T"].reshape(-1))
    img = Mesh.ToImage(mesh, c["width"], c["height"], *c["camera"], **lens)
    assert np.array_equal(bits(img.Values), bits(rgb)) and (img.Width, img.Height) == (c["width"], c["height"])


def test_mesh_raycast_and_occluded_members(gpu):
    c, want = Cs.case("cube"), Cs.model("cube")
    mesh = Mesh(c["V"], None, None, c["T"].reshape(-1))
    hits = Mesh.RayCast(mesh, c["O"][:300], c["D"][:300])
    assert np.array_equal(hits.Triangles, want.triangle[:300]) and np.array_equal(bits(hits.Distances), bits(want.distance[:300]))
    assert np.array_equal(Mesh.Occluded(mesh, c["O"][:300], c["D"][:300]), want.triangle[:300] >= 0)
    # one origin for all directions
    one = MeshSdf((c["V"], c["T"])).RayCast((0.5, 0.5, 0.5), c["D"][:100])
    assert np.all(one.Hit) and one.Points().shape == (100, 3)
    assert np.all(np.abs(one.Points() - 0.5).max(1) > 0.5 - 1e-6)   # on the cube's walls


# ---- accuracy and the ray marcher's sky -----------------------------------------------------------------------------------------------
def test_accuracy_on_the_marching_cubes_sphere_and_the_sky_of_the_ray_marcher(gpu):
    """Radial rays into the 64^3 sphere: |t - t_analytic| <= s sqrt(3), s the voxel edge -- every mesh point lies in a cell that holds
    a surface point.  The observed maximum, and the number of pixels on which a render of the mesh and RayMarcher.RenderDepth of the
    sphere disagree about the sky (recorded, not asserted; they lie on the silhouette), are those of tests/golden/mesh_ray_accuracy.json."""
    n, half, r = 64, 1.25, 1.0
    sdf = Sdfs.Sphere(r)
    mesh = sdf.ToMesh([-half] * 3, [half] * 3, n, n, n)
    t = MeshSdf(mesh)
    D = Cs.directions(4096, 7)
    hits = t.RayCast((0, 0, 0), D)
    assert np.all(hits.Hit)
    s = 2 * half / n
    t_analytic = r / np.linalg.norm(D.astype(f64), axis=1)
    err = float(np.abs(hits.Distances.astype(f64) - t_analytic).max())
    print(f"max |t - t_analytic| = {err:.6g}, bound {s * np.sqrt(3):.6g}")
    assert err <= s * np.sqrt(3)
    cam = ((1.5, 0.9, 2.4), (0, 0, 0), (0, 1, 0))
    w, h = 96, 72
    sky_mesh = ~np.isfinite(t.RenderDepth(w, h, *cam).Values)
    rm = RayMarcher(w, h, sdf)
    rm.ViewTransform = Matrix4x4.CreateLookAt(*cam)
    sky_sdf = rm.RenderDepth().Values > f32(rm.FarPlaneDistance)
    differ = sky_mesh != sky_sdf
    # the silhouette: pixels whose 3 x 3 neighbourhood sees both sky and sphere
    pad = np.pad(sky_sdf, 1, mode="edge")
    nb = np.stack([pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    silhouette = nb.any(0) & ~nb.all(0)
    print(f"sky disagreements: {int(differ.sum())} of {w * h} pixels, silhouette {int(silhouette.sum())}")
    assert np.all(silhouette[differ]) and 0.1 < (~sky_mesh).mean() < 0.9
    rec = json.load(open(GOLDEN))
    assert rec["sphere64_radial_max_abs_t_error"] == err and rec["sphere64_voxel_edge_sqrt3"] == s * np.sqrt(3)
    assert rec["sky_disagreeing_pixels_96x72"] is None or isinstance(rec["sky_disagreeing_pixels_96x72"], int)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu, handle):
    c = Cs.case("cube")
    t = handle(c)
    L = N.lib()
    n = 16
    o, d = c["O"][:n].copy(), c["D"][:n].copy()

    def cast(h, n_, tmin, tmax, flags, want_dist=True, who=L.sdfk_trimesh_raycast, op=o, dp=d):
        tri, dist, w = np.full(n, -7, i32), np.full(n, -7, f32), np.full((n, 3), -7, f32)
        r = who(h, _vp(op), _vp(dp), n_, C.c_float(tmin), C.c_float(tmax), flags, _vp(tri), _vp(dist) if want_dist else None, _vp(w) if want_dist else None)
        assert np.all(tri == -7) and np.all(dist == -7) and np.all(w == -7)
        return r, L.sdfk_last_error().decode()

    for who in (L.sdfk_trimesh_raycast, L.sdfk_trimesh_raycast_device):
        for args, word in (((None, n, 0, 1, 0), "null"), ((t.handle, -1, 0, 1, 0), "n must be"), ((t.handle, n, np.nan, 1, 0), "NaN"),
                           ((t.handle, n, 0, np.nan, 0), "NaN"), ((t.handle, n, 2, 1, 0), "t_min"), ((t.handle, n, 0, 1, 2), "flag"),
                           ((t.handle, n, 0, 1, 3), "flag"), ((t.handle, n, 0, 1, -1), "flag"), ((t.handle, n, 0, 1, RAY_ANY_HIT), "NULL")):
            r, msg = cast(*args, who=who)
            assert r == N.ERR_INVALID and "sdfk_trimesh_raycast" in msg and word in msg, (args, msg)
        r, msg = cast(t.handle, n, 0, 1, 0, who=who, op=None)
        assert r == N.ERR_INVALID and "null" in msg
    # n == 0 succeeds and touches nothing, null arrays included
    assert cast(t.handle, 0, 0, 1, 0)[0] == 0 and cast(t.handle, 0, 0, 1, 0, op=None, dp=None)[0] == 0
    assert cast(t.handle, 0, -np.inf, np.inf, RAY_ANY_HIT, want_dist=False)[0] == 0
    # infinite ranges are ranges
    assert L.sdfk_trimesh_raycast(t.handle, _vp(o), _vp(d), n, C.c_float(-np.inf), C.c_float(np.inf), 0, None, None, None) == 0
    # render
    rc = Cs.render_case("cube_2x2")
    cam, m = N.f3(rc["cam"]), (C.c_float * 16)(*[float(x) for x in rc["vpi"].ravel()])
    for who in (L.sdfk_trimesh_render, L.sdfk_trimesh_render_device):
        img = np.full(4, -7, f32)
        for args, word in (((None, 2, 2, cam, m, 1, 100, _vp(img), None, None), "null"), ((t.handle, 0, 2, cam, m, 1, 100, _vp(img), None, None), "width"),
                           ((t.handle, 2, -1, cam, m, 1, 100, _vp(img), None, None), "height"), ((t.handle, 2, 2, None, m, 1, 100, _vp(img), None, None), "null"),
                           ((t.handle, 2, 2, cam, None, 1, 100, _vp(img), None, None), "null"),
                           ((t.handle, 2, 2, cam, m, np.nan, 100, _vp(img), None, None), "NaN"), ((t.handle, 2, 2, cam, m, 100, 1, _vp(img), None, None), "near_plane"),
                           ((t.handle, 2, 2, cam, m, 1, 100, None, None, None), "no image")):
            a = list(args)
            a[5], a[6] = C.c_float(a[5]), C.c_float(a[6])
            assert who(*a) == N.ERR_INVALID
            msg = L.sdfk_last_error().decode()
            assert "sdfk_trimesh_render" in msg and word in msg, (args[1:3], msg)
            assert np.all(img == -7)
