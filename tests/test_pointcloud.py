"""CPU checks of point-cloud normals and volumes: the numpy model (tests/pointcloud_model.py) on cases derivable by hand, the
shared arithmetic of the kernels (sdfkit_amd/csrc/points_normals.h) built with g++ against the model bit for bit, the recorded
accuracy figures (tests/golden/pointcloud_accuracy.json), and the four new C-ABI entry points: exported, and refusing to run
without a device."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sdfkit_amd import _native as N
from tests import pointcloud_model as PC
from tests import points_knn_model as KM

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pointcloud_accuracy.json")
ENTRY_POINTS = ["sdfk_points_normals", "sdfk_points_normals_device", "sdfk_points_to_volume", "sdfk_points_to_volume_device"]


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def _plane(n=8, z=2.0):
    g = np.arange(n, dtype=f32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), np.full(n * n, z, f32)], axis=1)


# ---- normals: the model on hand-made cases ----
@pytest.mark.parametrize("k", [4, 8, 9, 16])   # (k = 3 on a lattice edge is the point and two collinear neighbours)
def test_lattice_plane_normals_are_exact(k):
    P = _plane()
    nrm, var = PC.normals(P, k)
    assert (nrm == np.array([0, 0, 1], f32)).all() and (var == 0).all()
    nrm, var = PC.normals(P, k, viewpoint=[3.0, 3.0, -5.0])          # a viewpoint below the plane
    assert (nrm == np.array([0, 0, -1], f32)).all() and (var == 0).all()
    per_point = np.tile(np.array([[3.0, 3.0, 9.0]], f32), (len(P), 1))
    per_point[::2, 2] = -9.0
    nrm, _ = PC.normals(P, k, viewpoint=per_point)
    assert (nrm[::2, 2] == -1).all() and (nrm[1::2, 2] == 1).all() and (nrm[:, :2] == 0).all()
    nrm, _ = PC.normals(P, k, viewpoint=[3.0, 3.0, 2.0])             # in the plane: d == 0 exactly, the rule without viewpoint
    assert (nrm == np.array([0, 0, 1], f32)).all()


def test_normals_degenerate_neighbourhoods():
    # duplicates only: the trace is 0
    P = np.concatenate([np.tile(np.array([[1, 2, 3]], f32), (5, 1)), _plane() + f32(100)])
    nrm, var = PC.normals(P, 4)
    assert (nrm[:5] == 0).all() and (var[:5] == 0).all() and (nrm[5:, 2] == 1).all()
    # fewer than three neighbours within max_distance
    P = np.concatenate([_plane(), np.array([[50, 50, 50], [50.5, 50, 50]], f32)])
    nrm, var = PC.normals(P, 8, max_distance=1.5)
    assert (nrm[-2:] == 0).all() and (var[-2:] == 0).all() and (nrm[:-2, 2] == 1).all()
    # duplicates count as neighbours: a point, its copy and two more span a plane
    P = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [9, 9, 9]], f32)
    nrm, var = PC.normals(P, 4)
    assert (nrm[:4] == np.array([0, 0, 1], f32)).all() and (var[:4] == 0).all()


def test_normals_collinear_neighbours_are_deterministic_and_perpendicular():
    P = np.stack([np.arange(10, dtype=f32), np.zeros(10, f32), np.zeros(10, f32)], axis=1)
    nrm, var = PC.normals(P, 5)
    assert (nrm[:, 0] == 0).all() and (var == 0).all()                # two zero eigenvalues: the lowest column, the y axis
    assert (nrm == np.array([0, 1, 0], f32)).all()
    again, _ = PC.normals(P, 5)
    assert np.array_equal(_bits(nrm), _bits(again))


def test_normals_of_a_sphere_are_radial_and_unit():
    P = _fibonacci(400)
    nrm, var = PC.normals(P, 10, viewpoint=[0, 0, 0])
    assert (np.einsum("ij,ij->i", nrm, P) < -0.99).all()              # towards the centre
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1, atol=1e-7) and (var >= 0).all() and (var < 0.05).all()


# ---- volumes: the model on hand-made cases ----
def test_plane_volume_is_exactly_z_minus_2():
    P = _plane()
    Nn = np.tile(np.array([[0, 0, 1]], f32), (len(P), 1))
    # k = 1 (the tangent plane of the nearest point): exact for every dyadic centre
    v, known = PC.to_volume(P, Nn, (-0.5, -0.5, 0), (7.5, 7.5, 4), (16, 16, 8), k=1)
    z = PC.centres((-0.5, -0.5, 0), (7.5, 7.5, 4), (16, 16, 8))[:, 2].reshape(16, 16, 8)
    assert known.all() and np.array_equal(_bits(v), _bits(z - f32(2)))
    # k = 8: every neighbour says the same e = z - 2, and sum(w e) / sum(w) == e exactly when the products w e are exact, i.e. for
    # e a power of two: centres at z = 2 -+ 0.25
    v, known = PC.to_volume(P, Nn, (-0.5, -0.5, 1.5), (7.5, 7.5, 2.5), (16, 16, 2), k=8)
    z = PC.centres((-0.5, -0.5, 1.5), (7.5, 7.5, 2.5), (16, 16, 2))[:, 2].reshape(16, 16, 2)
    assert known.all() and np.array_equal(_bits(v), _bits(z - f32(2))) and set(np.unique(v)) == {f32(-0.25), f32(0.25)}
    # ... and with a band that leaves only those centres known in a taller volume; the others are +-band by the fill
    v, known = PC.to_volume(P, Nn, (-0.5, -0.5, 0), (7.5, 7.5, 4), (16, 16, 8), k=8, max_distance=0.5)
    z = PC.centres((-0.5, -0.5, 0), (7.5, 7.5, 4), (16, 16, 8))[:, 2].reshape(16, 16, 8)
    assert known.any() and not known.all() and (np.abs(z[known] - 2) == 0.25).all()
    assert np.array_equal(_bits(v[known]), _bits((z - f32(2))[known]))
    assert (v[~known] == np.where(z[~known] < 2, f32(-0.5), f32(0.5))).all()


def test_zero_normals_are_skipped():
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
    Nn = np.array([[0, 0, 0], [0, 0, 1], [-0.0, 0.0, -0.0]], f32)
    Q = np.array([[0.1, 0.1, 0.5]], f32)
    idx, _, found = KM.knn(P, Q, 3)
    value, known = PC.blend(P, Nn, Q, idx, found, 3, np.inf)
    assert known[0] and value[0] == f32(0.5)                          # only point 1 speaks; W == 0 (it is the k-th): its plane
    value, known = PC.blend(P, np.zeros_like(Nn), Q, idx, found, 3, np.inf)
    assert not known[0]
    v, known = PC.to_volume(P, np.zeros_like(Nn), (-1, -1, -1), (1, 1, 1), (2, 2, 2), k=3)
    assert not known.any() and (v == np.inf).all()                    # a volume without a known voxel: +max_distance


def test_k1_and_equal_distances_use_the_first_tangent_plane():
    # four points at the same distance from the query, tilted planes: k = 1 takes point 0's plane; k = 4 has h2 = every d2, so all
    # weights are 0 and the first neighbour's plane is used as well; k = 4 of 5 points blends the three nearer ones
    P = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], f32)
    Nn = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 0.6, 0.8], [0, 0, -1]], f32)
    Q = np.array([[0, 0, 0.5]], f32)
    for k in (1, 4):
        idx, _, found = KM.knn(P, Q, k)
        value, known = PC.blend(P, Nn, Q, idx, found, k, np.inf)
        assert known[0] and value[0] == f32(0.5) and idx[0, 0] == 0
    P5 = np.concatenate([P, [[0, 0, 3]]]).astype(f32)
    N5 = np.concatenate([Nn, [[0, 0, 1]]]).astype(f32)
    idx, _, found = KM.knn(P5, Q, 5)
    value, _ = PC.blend(P5, N5, Q, idx, found, 5, np.inf)
    e = np.array([0.5, 0.6 + 0.4, -0.6 + 0.4, -0.5])                        # equal weights: the mean of the four planes
    assert abs(float(value[0]) - e.mean()) < 1e-6
    # duplicates of the query itself: every d2 and h2 are 0
    Pd = np.tile(np.array([[0, 0, 0.5]], f32), (3, 1))
    idx, _, found = KM.knn(Pd, Q, 3)
    value, known = PC.blend(Pd, np.tile(np.array([[0, 0, 1]], f32), (3, 1)), Q, idx, found, 3, np.inf)
    assert known[0] and value[0] == 0


def test_fill_rule_on_a_hand_made_mask():
    s = np.zeros((4, 3, 5), np.int8)
    s[0, 0] = [0, -1, 0, 1, 0]      # leading: first above (-); between: last below (-); trailing: last below (+)
    s[0, 1] = [0, 0, 0, 0, 1]
    #  (0, 2): a fully unknown column -> along y from (0, 1): last known below in y, per z
    s[1, 1] = [1, 0, 0, -1, 0]      # slab 1: columns 0 and 2 unknown; column 0 has nothing below in y: the first above
    #  slab 2: fully unknown -> along x from slab 1;  slab 3 known at one voxel
    s[3, 2, 4] = -1
    f = PC.fill_signs(s)
    assert list(f[0, 0]) == [-1, -1, -1, 1, 1]
    assert list(f[0, 1]) == [1, 1, 1, 1, 1]
    assert list(f[0, 2]) == [1, 1, 1, 1, 1]
    assert list(f[1, 1]) == [1, 1, 1, -1, -1]
    assert list(f[1, 0]) == list(f[1, 1]) and list(f[1, 2]) == list(f[1, 1])
    assert (f[2] == f[1]).all()                                        # the last signed slab below in x
    assert (f[3] == -1).all()
    assert (PC.fill_signs(np.zeros((4, 3, 5), np.int8)) == 1).all()    # a fully unknown volume
    assert np.array_equal(PC.fill_signs(f), f)                         # nothing unknown: unchanged


def _fibonacci(n, radius=1.0):
    i = np.arange(n, dtype=np.float64) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    return (radius * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)).astype(f32)


@pytest.mark.parametrize("k", [1, 8])
def test_banded_volume_equals_the_clamped_unbanded_one(k):
    """With band b the result equals the +inf result clamped to +-b at every voxel whose k-th neighbour lies within b (there the
    neighbour set and the cut-off are the same)."""
    P = _fibonacci(300)
    Nn = P.copy()
    box = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), (12, 11, 13))
    b = f32(0.4)
    full, _ = PC.to_volume(P, Nn, *box, k=k)
    band, known = PC.to_volume(P, Nn, *box, k=k, max_distance=b)
    _, dist, found = KM.knn(P, PC.centres(*box), k, b)
    same = (found == k).reshape(box[2])
    assert same.any() and not same.all() and known[same].all()
    assert np.array_equal(_bits(band[same]), _bits(np.clip(full, -b, b)[same]))
    assert (np.abs(band) <= b).all()


# ---- the kernels' arithmetic, built for the host ----
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("points_normals_host")
    exe = str(d / "points_normals_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "points_normals_host.cpp"), "-o", exe])

    def run(mode, data, out_dtype):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        data.tofile(fin)
        p = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and f"points_normals_host {mode} ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
        return np.fromfile(fout, out_dtype)
    return run


def _neighbourhoods(rs, cases):
    """cases x 64 neighbour slots around a centre each: generic, near-planar, near-isotropic, collinear, lattice, far from the origin."""
    kind = rs.integers(0, 6, cases)
    centre = (rs.standard_normal((cases, 3)) * np.where(kind == 5, 1000.0, 1.0)[:, None]).astype(f32)
    off = rs.standard_normal((cases, 64, 3))
    off[kind == 1, :, 2] *= 1e-4                                       # near-planar
    off[kind == 2] /= np.linalg.norm(off[kind == 2], axis=-1, keepdims=True)   # on a sphere: near-isotropic
    off[kind == 3, :, 1:] = 0                                          # collinear
    off[kind == 4] = rs.integers(-2, 3, (int((kind == 4).sum()), 64, 3))       # lattice: ties, exact zeros
    nb = (centre[:, None, :] + off.astype(f32) * f32(0.1)).astype(f32)
    nb[:, 0] = centre                                                  # the point is its own neighbour
    m = rs.choice([0, 1, 2, 3, 4, 8, 9, 16, 33, 64], cases)
    return centre, nb, m.astype(np.int32)


@pytest.mark.parametrize("with_view", [False, True])
def test_host_normals_equal_the_model(host, with_view):
    rs = np.random.default_rng(11 + with_view)
    cases = 3000
    centre, nb, m = _neighbourhoods(rs, cases)
    view = (centre + rs.standard_normal((cases, 3)).astype(f32)).astype(f32)
    view[::7] = centre[::7]                                            # d == 0 exactly
    rows = np.concatenate([m[:, None].astype(f32), centre, view, nb.reshape(cases, -1)], axis=1).astype(f32)
    out = host("normals", np.concatenate([np.array([cases, with_view], f32), rows.reshape(-1)]), f32).reshape(cases, 4)
    P = np.concatenate([centre, nb.reshape(-1, 3)])
    idx = np.zeros((len(P), 64), np.int32)
    idx[:cases] = cases + np.arange(cases)[:, None] * 64 + np.arange(64)[None, :]
    found = np.zeros(len(P), np.int32)
    found[:cases] = m
    vp = None
    if with_view:
        vp = np.zeros((len(P), 3), f32)
        vp[:cases] = view
    nrm, var = PC.normals_from_neighbours(P, idx, found, vp)
    assert np.array_equal(_bits(out[:, :3]), _bits(nrm[:cases])) and np.array_equal(_bits(out[:, 3]), _bits(var[:cases]))
    assert (nrm[:cases][m < 3] == 0).all() and np.any(nrm[:cases][m >= 3] != 0)


@pytest.mark.parametrize("k,md", [(1, np.inf), (8, np.inf), (8, 0.25), (16, 0.3), (64, np.inf)])
def test_host_blend_equals_the_model(host, k, md):
    rs = np.random.default_rng(100 + k)
    cases = 500
    P = (rs.random((cases * 64, 3), dtype=f32) - f32(0.5)) * f32(0.5)
    P[:64 * 20] = P[0]                                                 # duplicates: every d2 equal
    Nn = rs.standard_normal((len(P), 3)).astype(f32)
    Nn[rs.random(len(P)) < 0.1] = 0                                    # skipped
    Q = (rs.random((cases, 3), dtype=f32) - f32(0.5)) * f32(0.5)
    Q[:10] = P[0]                                                      # h2 == 0
    # each case has its own 64 points; its neighbours: the k nearest of them within md, as the search orders them
    idx = np.full((cases, k), -1, np.int32)
    found = np.zeros(cases, np.int32)
    for c in range(cases):
        i, _, f = KM.knn(P[64 * c:64 * c + 64], Q[c:c + 1], k, md)
        idx[c, :f[0]] = i[0, :f[0]] + 64 * c
        found[c] = f[0]
    value, known = PC.blend(P, Nn, Q, idx, found, k, md)
    d2 = PC._d2(P, Q, idx)
    slots = np.zeros((cases, 64, 7), f32)
    j = np.maximum(idx, 0)
    slots[:, :k, 0:3], slots[:, :k, 3:6], slots[:, :k, 6] = P[j], Nn[j], d2
    rows = np.concatenate([found[:, None].astype(f32), Q, slots.reshape(cases, -1)], axis=1).astype(f32)
    out = host("blend", np.concatenate([np.array([cases, k, md], f32), rows.reshape(-1)]), f32).reshape(cases, 2)
    assert np.array_equal(out[:, 0] != 0, known)
    assert np.array_equal(_bits(out[known, 1]), _bits(value[known]))
    assert known.any() and ((~known).any() or np.isinf(md)) and (found < k).any() == (not np.isinf(md))


def test_host_fill_equals_the_model(host):
    rs = np.random.default_rng(7)
    for shape, density in [((4, 3, 5), 0.2), ((9, 7, 6), 0.02), ((5, 5, 5), 0.0), ((6, 4, 7), 1.0), ((1, 1, 9), 0.3), ((8, 1, 1), 0.3)]:
        s = np.where(rs.random(shape) < density, rs.choice([-1, 1], shape), 0).astype(np.int8)
        out = host("fill", np.concatenate([np.array(shape, np.int32), s.reshape(-1).astype(np.int32)]), np.int32)
        assert np.array_equal(out[:-1].reshape(shape), PC.fill_signs(s)) and out[-1] == int((s == 0).sum())


# ---- recorded accuracy ----
def accuracy_figures():
    """The model on a Fibonacci sphere (radius 1, 1000 points, analytic normals for the volume) in [-1.5, 1.5]^3 at 32^3, k = 8, a band
    of 3 voxels.  roundtrip_vertex_bound: how far from radius 1 a vertex may lie after sphere -> mesh -> points -> volume ->
    Redistance -> mesh at this grid (tests/test_gpu_pointcloud.py), as a sum of what each step can add, h the voxel size:
      h / 2   the first mesh's vertices: on grid edges whose ends have different signs of the exact distance;
      h / 2   the mesher's inherited scale (vertex positions use N - 1 cells where sampling used N): up to half a voxel at the walls;
      E       the volume's values against the distance to the cloud near the surface, measured here on the Fibonacci cloud (the
              mesh's vertices are denser, and the flatter a neighbourhood the smaller the tangent-plane error);
      1.5 h   Redistance keeps every sign, so a vertex of the second mesh sits on an edge whose ends have different signs of the
              volume: both ends within E + h of the cloud, the vertex within h / 2 of one of them;
      h / 2   the mesher's scale again.
    In all E + 3 h."""
    P = _fibonacci(1000)
    analytic = P.astype(np.float64) / np.linalg.norm(P.astype(np.float64), axis=1, keepdims=True)
    nrm, _ = PC.normals(P, 8)
    cosang = np.clip(np.abs(np.einsum("ij,ij->i", nrm.astype(np.float64), analytic)), 0, 1)
    ang = np.degrees(np.arccos(cosang))
    shape, h = (32, 32, 32), 3.0 / 32
    band = f32(3 * h)
    v, known = PC.to_volume(P, analytic.astype(f32), (-1.5,) * 3, (1.5,) * 3, shape, k=8, max_distance=band)
    truth = np.linalg.norm(PC.centres((-1.5,) * 3, (1.5,) * 3, shape).astype(np.float64), axis=1).reshape(shape) - 1.0
    near = np.abs(truth) <= float(band) / 2
    assert known[near].all()
    err = float(np.abs(v.astype(np.float64) - truth)[near].max())
    wrong = int(((v < 0) != (truth < 0))[~known].sum())
    return {"points": 1000, "grid": 32, "k": 8, "band_voxels": 3,
            "normal_angle_max_deg": round(float(ang.max()), 6), "normal_angle_mean_deg": round(float(ang.mean()), 6),
            "value_error_max_voxels": round(err / h, 6), "wrong_far_signs": wrong,
            "roundtrip_vertex_bound": round(err + 3 * h, 6)}


def test_recorded_accuracy_figures_are_the_models():
    fig = accuracy_figures()
    assert fig["wrong_far_signs"] == 0                                 # a condition, not a measurement
    with open(GOLDEN) as f:
        assert json.load(f) == fig


# ---- the C ABI ----
def test_pointcloud_entry_points_exported():
    L = N.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in N.SIGNATURES, name


def test_pointcloud_refuse_without_device():
    """No device (or sdfk_init not called): every new entry point returns SDFK_ERR_NO_DEVICE, in a fresh process."""
    p = subprocess.run([sys.executable, "-c", "from tests.test_pointcloud import _refusals; _refusals(); print('refusals ok')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "refusals ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def _refusals():
    L = N.lib()
    a = np.zeros((3, 3), f32)
    A = C.c_void_p(a.ctypes.data)
    calls = {
        "sdfk_points_normals": lambda: L.sdfk_points_normals(None, 8, np.inf, None, 0, A, None),
        "sdfk_points_normals_device": lambda: L.sdfk_points_normals_device(None, 8, np.inf, None, 0, A, None),
        "sdfk_points_to_volume": lambda: L.sdfk_points_to_volume(None, A, None, 8, np.inf, None),
        "sdfk_points_to_volume_device": lambda: L.sdfk_points_to_volume_device(None, A, None, 8, np.inf, None),
    }
    assert sorted(calls) == sorted(ENTRY_POINTS)
    for name, call in calls.items():
        assert call() == N.ERR_NO_DEVICE, name
