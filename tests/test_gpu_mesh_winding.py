"""The generalized winding number on the device (sdfk_trimesh_winding / sdfk_trimesh_to_volume_signed, csrc/lib_trimesh_winding.hip)
through the Python layers, against the numpy model (tests/mesh_winding_model.py) bit for bit: every case of
tests/mesh_winding_cases.py, host and device forms; the profiled term counts against the host program's (tests/cpp/
mesh_winding_host.cpp runs the same walk: equal counts mean the device ran it too); PARITY through the new entry point against
sdfk_trimesh_to_volume, whole, as a slab and with a band; WINDING against PARITY on closed meshes and against the union of the two
overlapping cubes; the repair of a sphere with its cap cut off; the reuse of a handle; the refusals; NaN queries."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from sdfkit_amd import Mesh
from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import DEFAULT_WINDING_BETA, MeshSdf
from tests import mesh_winding_cases as Cs
from tests import meshsdf_model as MM

pytestmark = pytest.mark.gpu

f32, f64, u32, i32 = np.float32, np.float64, np.uint32, np.int32
PARITY, WINDING = 0, 1


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_winding_gpu")
    return Cs.build_host(d), d


@pytest.fixture(scope="module")
def handle(gpu):
    """handle(case) -> one MeshSdf per mesh of the cases; all are freed when the module is done"""
    made = {}

    def get(c):
        key = (c["V"].tobytes(), c["T"].tobytes())
        if key not in made:
            made[key] = MeshSdf((c["V"], c["T"]))
        return made[key]

    yield get
    for t in made.values():
        t.__del__()
    made.clear()


def signed_volume(t, c, mode, beta=DEFAULT_WINDING_BETA, band=None, slab=True):
    """sdfk_trimesh_to_volume_signed (mode None: sdfk_trimesh_to_volume) into the case's volume -> (values, colours)"""
    L = N.lib()
    n = c["n"]
    z0, nz = (c["z0"], c["nz"]) if slab else (0, n[2])
    h = C.c_void_p()
    N.check(L.sdfk_volume_create_slab(n[0], n[1], n[2], N.f3(c["mn"]), N.f3(c["mx"]), z0, nz, 1, C.byref(h)))
    try:
        b = C.c_float(c["band"] if band is None else band)
        if mode is None:
            N.check(L.sdfk_trimesh_to_volume(t.handle, h, b))
        else:
            N.check(L.sdfk_trimesh_to_volume_signed(t.handle, h, b, mode, C.c_float(beta)))
        vals, cols = np.empty((n[0], n[1], nz), f32), np.empty((n[0], n[1], nz, 3), f32)
        N.check(L.sdfk_volume_download(h, _vp(vals), _vp(cols)))
    finally:
        L.sdfk_volume_free(h)
    return vals, cols


# ---- point queries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.CASES))
def test_winding_equals_model_bit_for_bit(gpu, handle, host, name):
    exe, d = host
    c, want = Cs.case(name), Cs.model(name)
    t = handle(c)
    n = len(c["Q"])
    w, inside = np.full(n + 1, -7, f32), np.full(n + 1, 7, np.uint8)
    N.check(N.lib().sdfk_profile_enable(1))
    try:
        N.check(N.lib().sdfk_trimesh_winding(t.handle, _vp(c["Q"]), n, C.c_float(DEFAULT_WINDING_BETA), _vp(w), _vp(inside)))
        s = t.winding_stats()
    finally:
        N.check(N.lib().sdfk_profile_enable(0))
    assert w[n] == -7 and inside[n] == 7                      # nothing past the end
    assert np.array_equal(bits(w[:n]), bits(want.winding)), np.flatnonzero(bits(w[:n]) != bits(want.winding))[:8]
    assert np.array_equal(inside[:n].astype(bool), want.inside)
    # the members, and either output alone
    assert np.array_equal(bits(t.WindingNumber(c["Q"])), bits(want.winding)) and np.array_equal(t.Contains(c["Q"]), want.inside)
    # the hierarchy and the profiled term counts: the host program's, which runs the same walk
    h = Cs.host_run(exe, d, c["V"], c["T"], c["Q"], DEFAULT_WINDING_BETA)
    assert (s["levels"], s["occupied_nodes"], s["largest_leaf"], s["builds"]) == (h.L, h.occupied, h.max_leaf, 1)
    assert (s["cluster_terms"], s["triangle_terms"], s["queries"]) == (h.cluster_terms, h.triangle_terms, n)


@pytest.mark.parametrize("beta", [0.0, 1.0, np.inf])
def test_other_betas(gpu, handle, beta):
    for name in ("two_cubes", "hemisphere"):
        c, want = Cs.case(name), Cs.model(name, beta)
        t = handle(c)
        assert np.array_equal(bits(t.WindingNumber(c["Q"], beta)), bits(want.winding)) and np.array_equal(t.Contains(c["Q"], beta), want.inside)


def test_device_form(gpu, handle):
    import torch
    c, want = Cs.case("big_sphere"), Cs.model("big_sphere")
    t = handle(c)
    dev = torch.device("cuda", N.init())
    n = len(c["Q"])
    q = torch.from_numpy(c["Q"].copy()).to(dev)
    for sel in ((1, 1), (1, 0), (0, 1)):
        w = torch.full((n + 1,), -7.0, dtype=torch.float32, device=dev)
        inside = torch.full((n + 1,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        t.WindingNumberDevice(q.data_ptr(), n, DEFAULT_WINDING_BETA, w.data_ptr() if sel[0] else None, inside.data_ptr() if sel[1] else None)
        N.check(N.lib().sdfk_synchronize())
        w, inside = w.cpu().numpy(), inside.cpu().numpy()
        assert w[-1] == -7 and inside[-1] == 7
        assert np.array_equal(bits(w[:-1]), bits(want.winding)) if sel[0] else np.all(w == -7)
        assert np.array_equal(inside[:-1].astype(bool), want.inside) if sel[1] else np.all(inside == 7)


def test_nan_queries_and_mesh_members(gpu):
    c, want = Cs.case("bad_queries"), Cs.model("bad_queries")
    m = Mesh(c["V"], None, None, c["T"].reshape(-1))
    w = m.WindingNumber(c["Q"])
    bad = ~np.all(np.isfinite(c["Q"]), 1)
    assert np.array_equal(bits(w), bits(want.winding)) and np.all(np.isnan(w[bad])) and np.all(bits(w[bad]) == 0x7fc00000)
    inside = m.Contains(c["Q"])
    assert np.array_equal(inside, want.inside) and not inside[bad].any() and inside[4]


def test_handle_is_reusable_and_the_hierarchy_is_built_once(gpu):
    c = Cs.case("sphere_cap_removed")
    t = MeshSdf((c["V"], c["T"]))
    assert t.winding_stats()["levels"] == -1 and t.winding_stats()["builds"] == 0
    a = t.WindingNumber(c["Q"])
    tri, dist, _ = t.Search(c["Q"][:64])                      # the other queries of the handle still work in between
    b = t.WindingNumber(c["Q"])
    vals, _ = signed_volume(t, c, WINDING)
    s = t.winding_stats()
    assert s["builds"] == 1 and s["levels"] == Cs.tree("sphere_cap_removed").L and s["nodes"] == Cs.tree("sphere_cap_removed").total
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(Cs.model("sphere_cap_removed").winding))
    assert np.all(tri >= 0) and np.all(np.isfinite(dist))


# ---- volumes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "big_sphere", "banded_cube", "cube_no_lid", "two_cubes"])
def test_parity_mode_is_to_volume_bit_for_bit(gpu, handle, name):
    """whole, as a slab (big_sphere: z0 = 8) and with a band (big_sphere, banded_cube), values and colours; open and overlapping
    meshes too: the parity sign is deterministic there"""
    c = Cs.case(name)
    t = handle(c)
    for slab in (True, False):
        for band in (None, np.inf):
            want = signed_volume(t, c, None, band=band, slab=slab)
            got = signed_volume(t, c, PARITY, band=band, slab=slab)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
            assert (want[0] < 0).any() and (want[0] > 0).any()


@pytest.mark.parametrize("name", list(Cs.CASES))
def test_winding_volume_sign_equals_model_and_distances_equal_parity(gpu, handle, host, name):
    """every voxel: the magnitude (and the colours) of the PARITY volume, the sign of the model at the f32 cell centre"""
    exe, d = host
    c = Cs.case(name)
    t = handle(c)
    par, pcol = signed_volume(t, c, PARITY)
    N.check(N.lib().sdfk_profile_enable(1))
    try:
        win, wcol = signed_volume(t, c, WINDING)
        s, crossings = t.winding_stats(), t.stats()["crossings"]
    finally:
        N.check(N.lib().sdfk_profile_enable(0))
    inside = Cs.volume_model(name).inside.reshape(win.shape)
    assert np.array_equal(bits(np.abs(win)), bits(np.abs(par))) and np.array_equal(bits(wcol), bits(pcol))
    assert np.array_equal(np.signbit(win), inside)
    h = Cs.host_run(exe, d, c["V"], c["T"], Cs.voxel_centres(c), DEFAULT_WINDING_BETA, "vol")
    assert (s["cluster_terms"], s["triangle_terms"], s["queries"]) == (h.cluster_terms, h.triangle_terms, win.size)
    assert crossings == 0                                      # the crossing records are not built
    if name in Cs.CLOSED:                                      # WINDING is PARITY, bit for bit, wherever d > 0
        off = par != 0
        assert off.sum() > 0.9 * par.size and np.array_equal(bits(win[off]), bits(par[off])) and (par < 0).any()


def test_overlapping_cubes_union_not_xor(gpu, handle):
    c = Cs.case("two_cubes")
    t = handle(c)
    win, _ = signed_volume(t, c, WINDING)
    par, _ = signed_volume(t, c, PARITY)
    apart = [signed_volume(MeshSdf(MM.box_mesh(*box)), c, None)[0] for box in (Cs.TWO_A, Cs.TWO_B)]
    union = np.minimum(apart[0], apart[1])
    assert np.array_equal(np.signbit(win), np.signbit(union))
    both = (apart[0] < 0) & (apart[1] < 0)
    assert both.sum() > 50 and np.all(par[both] > 0) and not np.array_equal(np.signbit(par), np.signbit(union))
    assert np.array_equal(np.signbit(par), np.signbit(apart[0]) ^ np.signbit(apart[1]))     # parity: the XOR


def test_repair_of_the_capped_off_sphere(gpu):
    """ToVoxels(sign="winding", maxDistance=band) -> Redistance -> ToMesh: watertight, one component, and near the sphere.

    How near, derived and not tuned.  DX is the grid spacing, h the spacing of the grid the sphere was meshed on (the same here).
    The |w| = 1/2 surface of a sphere with a circular hole is the flat disc on the hole's rim; the rim lies within one mesh
    cell of z = CAP_Z (triangles were removed by centroid), so the disc lies at most (1 - CAP_Z) + h inside the unit sphere.
    Next to the cap the volume's magnitudes are distances to the mesh's triangles, not to the cap, so Redistance -- which takes the
    front from the input's own zero crossings -- may place the surface anywhere on the grid edges the sign changes across: 1 DX.
    Its recorded first-order shift of a front (tests/golden/redistance_accuracy.json, the largest edge_shift) adds 0.2022 DX.
    The marching-cubes sphere's own distance from the unit sphere, at most h^2 / 8 for a chord of length h, is covered by
    rounding 0.2022 up to 0.25."""
    c = Cs.case("sphere_cap_removed")
    with open(os.path.join(Cs.ROOT, "tests", "golden", "redistance_accuracy.json")) as f:
        acc = json.load(f)
    shifts = [acc["mesh"][k]["edge_shift"] for k in acc["mesh"]] + [r["edge_shift"] for g in acc["sphere"].values() for r in g.values()]
    assert max(shifts) <= 0.2022
    n = 24
    dx = h = 2.5 / n
    bound = (1 - Cs.CAP_Z) + h + (1 + 0.25) * dx
    mesh = Mesh(c["V"], None, None, c["T"].reshape(-1))
    before = mesh.Topology()
    assert not before.IsWatertight and before.BoundaryEdges > 10
    vox = mesh.ToVoxels([-1.25] * 3, [1.25] * 3, n, n, n, maxDistance=3 * dx, sign="winding")
    fixed = vox.Redistance().ToMesh()
    top = fixed.Topology()
    assert top.IsWatertight and top.Components == 1 and top.BoundaryEdges == 0 and top.Triangles > 1000
    r = np.linalg.norm(np.asarray(fixed.Vertices, f64).reshape(-1, 3), axis=1)
    print(f"repair: {top.Triangles} triangles, |v| in [{r.min():.4f}, {r.max():.4f}], allowed deviation {bound:.4f} ({bound / dx:.2f} voxels)")
    assert np.abs(r - 1).max() <= bound
    below = np.asarray(fixed.Vertices, f64).reshape(-1, 3)[:, 2] < 0.0                  # the half away from the hole: the sphere itself
    print(f"repair: in the half away from the hole | |v| - 1 | <= {np.abs(r[below] - 1).max() / dx:.3f} voxels over {below.sum()} vertices")
    assert below.sum() > 500
    # parity on the same mesh leaves streaks: its volume has sign changes the winding volume does not have
    par = mesh.ToVoxels([-1.25] * 3, [1.25] * 3, n, n, n, maxDistance=3 * dx).Values
    assert (np.signbit(par) != np.signbit(vox.Values)).sum() > 20


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu, handle):
    L = N.lib()
    c = Cs.case("cube")
    t = handle(c)
    n = len(c["Q"])
    w, inside = np.full(n, -7, f32), np.full(n, 7, np.uint8)
    beta = C.c_float(DEFAULT_WINDING_BETA)
    assert L.sdfk_trimesh_winding(None, _vp(c["Q"]), n, beta, _vp(w), _vp(inside)) == 1
    assert L.sdfk_trimesh_winding(t.handle, _vp(c["Q"]), -1, beta, _vp(w), _vp(inside)) == 1
    assert L.sdfk_trimesh_winding(t.handle, _vp(c["Q"]), 1 << 32, beta, _vp(w), _vp(inside)) == 1
    assert L.sdfk_trimesh_winding(t.handle, None, n, beta, _vp(w), _vp(inside)) == 1
    for bad in (-1.0, -0.0001, np.nan, -np.inf):
        assert L.sdfk_trimesh_winding(t.handle, _vp(c["Q"]), n, C.c_float(bad), _vp(w), _vp(inside)) == 1
        assert b"beta" in L.sdfk_last_error()
        assert L.sdfk_trimesh_winding_device(t.handle, _vp(c["Q"]), n, C.c_float(bad), None, None) == 1
    assert np.all(w == -7) and np.all(inside == 7)
    assert L.sdfk_trimesh_winding(t.handle, None, 0, beta, None, None) == 0          # n == 0: nothing is touched
    assert L.sdfk_trimesh_winding(t.handle, _vp(c["Q"]), n, beta, None, None) == 0     # no output asked for: fine
    assert L.sdfk_trimesh_winding_stats(None, (C.c_int64 * 8)()) == 1 and L.sdfk_trimesh_winding_stats(t.handle, None) == 1
    h = C.c_void_p()
    N.check(L.sdfk_volume_create_slab(4, 4, 4, N.f3([-1] * 3), N.f3([2] * 3), 0, 4, 0, C.byref(h)))
    try:
        one = C.c_float(1.0)
        assert L.sdfk_trimesh_to_volume_signed(None, h, one, WINDING, beta) == 1
        assert L.sdfk_trimesh_to_volume_signed(t.handle, None, one, WINDING, beta) == 1
        assert L.sdfk_trimesh_to_volume_signed(t.handle, h, C.c_float(-1.0), WINDING, beta) == 1
        assert L.sdfk_trimesh_to_volume_signed(t.handle, h, C.c_float(np.nan), PARITY, beta) == 1
        assert L.sdfk_trimesh_to_volume_signed(t.handle, h, one, 2, beta) == 1 and b"sign_mode" in L.sdfk_last_error()
        assert L.sdfk_trimesh_to_volume_signed(t.handle, h, one, -1, beta) == 1
        assert L.sdfk_trimesh_to_volume_signed(t.handle, h, one, WINDING, C.c_float(np.nan)) == 1
        assert L.sdfk_trimesh_to_volume_signed(t.handle, h, one, WINDING, C.c_float(-2.0)) == 1
        assert L.sdfk_trimesh_to_volume_signed(t.handle, h, one, PARITY, C.c_float(np.nan)) == 0     # PARITY ignores beta
        assert L.sdfk_trimesh_to_volume_signed(t.handle, h, one, WINDING, beta) == 0
    finally:
        L.sdfk_volume_free(h)
    with pytest.raises(ValueError):
        t.ToVoxels([-1] * 3, [2] * 3, 4, 4, 4, sign="nonzero")
