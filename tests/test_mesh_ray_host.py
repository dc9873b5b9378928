"""CPU proof of the mesh ray walk (sdfkit_amd/csrc/trimesh_ray.h, the very code the kernels of lib_trimesh_ray.hip run, built with
g++ -O2 -ffp-contract=off by tests/cpp/mesh_ray_host.cpp over a grid rebuilt as the library builds it) against the numpy model
(tests/mesh_ray_model.py, brute force over all triangles): every case of tests/mesh_ray_cases.py, bit for bit, first hit and any hit;
the camera rays and the shading of the render cases; what the hand-made cases are built to show; the pruning condition; and the same
program once more under -fsanitize=address,undefined (a stand-alone program: nothing is preloaded)."""
import numpy as np
import pytest

from tests import mesh_ray_cases as Cs
from tests import mesh_ray_model as M

f32, u32 = np.float32, np.uint32


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_ray")
    return Cs.build_host(d), d


@pytest.mark.parametrize("name", list(Cs.CASES))
def test_walk_equals_brute_force_model(host, name):
    exe, d = host
    c, want = Cs.case(name), Cs.model(name)
    head, tri, dist, w, per_ray = Cs.host_cast(exe, d, c)
    assert head["differs"] == 0                       # the header's own brute force, the same test: the walk missed nothing
    assert np.array_equal(tri, want.triangle), np.flatnonzero(tri != want.triangle)[:8]
    assert np.array_equal(bits(dist), bits(want.distance)) and np.array_equal(bits(w), bits(want.weights))
    print(f"{name}: {head['tests']} binary64 tests for {head['n']} rays over {len(c['T'])} triangles, grid {head['dim']}")
    # any hit: the same rays hit, and the walk stops no later
    head_any, tri_any, _, _, _ = Cs.host_cast(exe, d, c, M.ANY_HIT, "any")
    assert head_any["differs"] == 0 and np.array_equal(tri_any, Cs.model(name, M.ANY_HIT).triangle)
    assert np.array_equal(tri_any >= 0, want.triangle >= 0) and head_any["tests"] <= head["tests"]


@pytest.mark.parametrize("name", list(Cs.RENDER))
def test_render_equals_model(host, name):
    exe, d = host
    c = Cs.render_case(name)
    depth, rgb, tri = Cs.render_model(name)
    head, hd, hrgb, htri = Cs.host_render(exe, d, c)
    assert head["differs"] == 0 and np.array_equal(htri, tri)
    assert np.array_equal(bits(hd), bits(depth)) and np.array_equal(bits(hrgb), bits(rgb))


def test_what_the_cases_are_built_to_show():
    m = Cs.model
    for name in Cs.EVERY_RAY_HITS:
        assert np.all(m(name).triangle >= 0), name
    # the lowest index wins a tie: the perpendicular rays are exact, so a point of a shared edge or vertex lies in several triangles
    for name in Cs.EVERY_RAY_HITS:
        c = Cs.case(name)
        perp = (c["D"][:, 0] == 0) & (c["D"][:, 1] == 0)
        assert perp.sum() == 2 * 48
        want = Cs.lowest_containing(c["V"], c["T"], c["O"][perp])
        assert np.array_equal(m(name).triangle[perp], want) and len(set(want.tolist())) > 2, name
    # from the centre of a closed mesh every ray hits
    for name in Cs.CLOSED:
        c = Cs.case(name)
        centre = np.all(c["O"] == c["O"][0], 1)
        assert np.all(m(name).triangle[centre] >= 0), name
    out = ~np.all(Cs.case("sphere")["O"] == 0, 1)
    miss = (m("sphere").triangle[out] < 0).mean()
    assert 0.15 < miss < 0.6                           # "about half" of the random outside rays miss, the aimed ones hit
    assert m("early_exit_trap").triangle.tolist() == [1, 1, 1, 1, 0]   # (the last ray comes from the far side: the large one is first)
    assert m("thin_triangle").triangle.tolist()[:3] == [0, 0, 0] and m("thin_triangle").triangle[3] != 0
    st = m("single_triangle")
    assert np.all(st.triangle[-6:] == -1)              # parallel to the plane and in it
    assert (st.triangle >= 0).sum() > 40 and (st.triangle < 0).sum() > 10
    bad = M.bad_rays(Cs.case("bad_rays")["O"], Cs.case("bad_rays")["D"])
    assert bad.sum() == 20 and np.all(m("bad_rays").triangle[bad] == -1) and np.all(m("bad_rays").triangle[~bad] >= 0)
    # ranges around the hit at t = 0.5 (rays 0 and 1) and the wall behind at -0.5; ray 2 has |d| = 2: its hit is at 0.25
    hits = {n[6:]: (m(n).triangle[:2] >= 0).tolist() for n in Cs.CASES if n.startswith("range_")}
    assert hits == {"tmax_below": [False] * 2, "tmax_at": [True] * 2, "tmax_above": [True] * 2, "tmin_below": [True] * 2, "tmin_at": [True] * 2,
                    "tmin_above": [False] * 2, "point": [True] * 2, "to_inf": [True] * 2, "behind": [True] * 2, "behind_far": [True] * 2,
                    "all": [True] * 2}
    assert m("range_behind").distance[0] == f32(-0.5) and m("range_all").distance[0] == f32(-0.5) and m("range_to_inf").distance[2] == f32(0.25)
    # scaling the directions scales t inversely and keeps the triangle
    base = m("cube")
    for name, k in (("scale_1e-30", 1e30), ("scale_1e30", 1e-30)):
        s = m(name)
        assert np.array_equal(s.triangle, base.triangle[:600])
        assert np.allclose(s.distance.astype(np.float64), base.distance[:600].astype(np.float64) * k, rtol=1e-6)
    assert np.all(m("far_mesh").triangle[:400] >= 0)
    # render: the sky cases are all sky, the others see the mesh, and near beyond the front wall shows the back wall
    assert np.all(Cs.render_model("far_all_sky")[2] == -1) and np.all(Cs.render_model("cube_1x1")[2] == -1)
    assert (Cs.render_model("sphere_64x48")[2] >= 0).mean() > 0.1 and np.all(Cs.render_model("inside_sphere")[2] >= 0)
    d = Cs.render_model("near_past_front")[0]
    assert np.isfinite(d).any() and d[np.isfinite(d)].min() >= 4.5


def test_the_walk_prunes(host):
    """The condition of the device test, met first here: fewer binary64 tests than a tenth of brute force's rays x triangles."""
    exe, d = host
    c = Cs.case("sphere_inside_random")
    head, *_ = Cs.host_cast(exe, d, c)
    assert head["tests"] < head["n"] * len(c["T"]) / 10, head
    assert head["tests"] < head["n"] * 200, head


def test_host_program_under_sanitizers(tmp_path):
    exe = Cs.build_host(tmp_path, sanitize=True)
    for name in ("walk_traps", "early_exit_trap", "flat_mesh", "bad_rays", "far_mesh", "count_0"):
        c = Cs.case(name)
        head, tri, *_ = Cs.host_cast(exe, tmp_path, c)
        assert head["differs"] == 0 and np.array_equal(tri, Cs.model(name).triangle)
    c = Cs.render_case("sphere_colors_1x7")
    head, _, _, tri = Cs.host_render(exe, tmp_path, c)
    assert np.array_equal(tri, Cs.render_model("sphere_colors_1x7")[2])
