"""CPU proof of the winding-number sum (sdfkit_amd/csrc/trimesh_winding.h, the very code the kernels of lib_trimesh_winding.hip run,
built with g++ -O2 -ffp-contract=off by tests/cpp/mesh_winding_host.cpp over a hierarchy rebuilt as the library builds it) against
the numpy model (tests/mesh_winding_model.py): every case of tests/mesh_winding_cases.py bit for bit -- the nodes, w, inside and the
term counts; beta = +inf against the same code's brute loop; what the cases are built to show; the recorded accuracy against brute force
with np.arctan2 (tests/golden/mesh_winding_accuracy.json), on which the default beta rests; and the same program once more under
-fsanitize=address,undefined (a stand-alone program: nothing is preloaded)."""
import numpy as np
import pytest

from tests import mesh_winding_cases as Cs
from tests import mesh_winding_model as M

f32, f64, i64 = np.float32, np.float64, np.int64


def bits(a):
    return np.ascontiguousarray(a, f64).view(i64)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_winding")
    return Cs.build_host(d), d


def same_answer(h, want):
    assert np.array_equal(bits(h.w), bits(want.w)), np.flatnonzero(bits(h.w) != bits(want.w))[:8]
    assert np.array_equal(h.inside, want.inside)
    assert np.array_equal(h.clusters, want.clusters) and np.array_equal(h.triangles, want.triangles)


@pytest.mark.parametrize("name", list(Cs.CASES))
def test_walk_equals_model(host, name):
    exe, d = host
    c, H, want = Cs.case(name), Cs.tree(name), Cs.model(name)
    h = Cs.host_run(exe, d, c["V"], c["T"], c["Q"], Cs.DEFAULT_BETA)
    assert (h.L, h.occupied, h.max_leaf) == (H.L, H.occupied, H.max_leaf)
    occ = H.count > 0
    assert np.array_equal(h.count, H.count) and np.array_equal(h.start[occ], H.start[occ])
    assert np.array_equal(bits(h.N), bits(H.N)) and np.array_equal(bits(h.P), bits(H.P)) and np.array_equal(bits(h.r2), bits(H.r2))
    same_answer(h, want)
    assert h.differs == 0                      # beta = +inf: the walk is the same code's brute loop, bit for bit
    assert h.cluster_terms == want.clusters.sum() and h.triangle_terms == want.triangles.sum()
    print(f"{name}: L {h.L}, {h.occupied} nodes, {h.cluster_terms} cluster + {h.triangle_terms} triangle terms for {len(c['Q'])} queries "
          f"over {len(c['T'])} triangles")


@pytest.mark.parametrize("beta", [0.0, 1.0, 4.0, np.inf])
def test_other_betas(host, beta):
    exe, d = host
    for name in ("two_cubes", "hemisphere"):
        c = Cs.case(name)
        want = Cs.model(name, beta)
        same_answer(Cs.host_run(exe, d, c["V"], c["T"], c["Q"], beta), want)
        fin = np.all(np.isfinite(c["Q"]), 1)
        if beta == 0.0:
            assert np.all(want.clusters[fin] == 1) and not want.triangles.any()
        if beta == np.inf:
            assert not want.clusters.any() and np.all(want.triangles[fin] == len(c["T"]))
            assert np.array_equal(bits(want.w), bits(M.sorted_brute(Cs.tree(name), c["Q"])))


def test_volume_queries_equal_model(host):
    """the cell centres of a slab with z0 > 0 and of a volume whose nz is no multiple of 64, as the sign pass forms them"""
    exe, d = host
    for name in ("big_sphere", "two_cubes"):
        c = Cs.case(name)
        same_answer(Cs.host_run(exe, d, c["V"], c["T"], Cs.voxel_centres(c), Cs.DEFAULT_BETA), Cs.volume_model(name))


def test_what_the_cases_are_built_to_show():
    rec = Cs.recorded()["cases"]
    # closed meshes: w is an integer to within the recorded error, +1 / -1 inside by the orientation, Contains unchanged
    for name in ("cube", "octahedron", "nested_shells", "big_sphere"):
        w = Cs.volume_model(name).w
        assert np.abs(w - np.rint(w)).max() <= rec[name][repr(Cs.DEFAULT_BETA)]["max_error"] + 1e-12, name
    for name in ("cube", "octahedron"):
        # (off the surface, and to rounding: on the surface the sign of a term is that of a zero or of rounding noise, and
        # reversing a triangle's vertices reorders the products of its denominator)
        va, vb = Cs.volume_model(name), Cs.volume_model(name + "_inside_out")
        assert np.abs(va.w + vb.w).max() <= 1e-14
        assert np.array_equal(va.inside, vb.inside) and va.inside.any() and np.all(np.rint(va.w[va.inside]) == 1) and np.all(np.rint(vb.w[vb.inside]) == -1)
    # the overlap of the two cubes has w = 2; inside is the union, where parity would give the XOR
    c = Cs.case("two_cubes")
    P = Cs.voxel_centres(c).astype(f64)
    in_a = np.all((P > Cs.TWO_A[0]) & (P < Cs.TWO_A[1]), 1)
    in_b = np.all((P > Cs.TWO_B[0]) & (P < Cs.TWO_B[1]), 1)
    v = Cs.volume_model("two_cubes")
    assert (in_a & in_b).sum() > 50 and np.all(np.rint(v.w[in_a & in_b]) == 2) and np.all(np.rint(v.w[in_a ^ in_b]) == 1)
    assert np.array_equal(v.inside, in_a | in_b)
    # the cavity of the nested shells has w = 0
    c = Cs.case("nested_shells")
    P = Cs.voxel_centres(c).astype(f64)
    cavity, outer = np.all((P > 1) & (P < 2), 1), np.all((P > 0) & (P < 3), 1)
    v = Cs.volume_model("nested_shells")
    assert cavity.sum() > 20 and np.all(np.rint(v.w[cavity]) == 0) and np.array_equal(v.inside, outer & ~cavity)
    # every triangle twice: w = 2 inside; the zero-area triangles add nothing off their own segments
    d = Cs.case("degenerate")
    inside_octa = np.abs(d["Q"].astype(f64) - [0.25, -0.5, 0.125]).sum(1) < 0.999
    assert inside_octa.sum() > 10 and np.all(np.rint(Cs.model("degenerate").w[inside_octa]) == 2)
    assert abs(Cs.model("degenerate").w[-1]) < 1e-9            # beside the collinear triangle
    assert np.all(np.isfinite(Cs.model("degenerate").w))         # on it, and at its vertices, too
    # L >= 2, and both ends of the walk: some queries open every level, some stop at the root
    H, m = Cs.tree("big_sphere"), Cs.model("big_sphere")
    assert H.L >= 2 and np.any((m.clusters == 1) & (m.triangles == 0)) and np.any(m.triangles > 0)
    # bad queries: NaN, not inside
    b = Cs.model("bad_queries")
    bad = ~np.all(np.isfinite(Cs.case("bad_queries")["Q"]), 1)
    assert bad.sum() == 5 and np.all(np.isnan(b.w[bad])) and not b.inside[bad].any() and np.all(np.isfinite(b.w[~bad]))
    assert b.inside[4] and not b.inside[6] and not b.inside[7]
    assert np.array_equal(b.winding[bad].view(np.uint32), np.full(5, 0x7fc00000, np.uint32))
    # a query equal to a vertex, on an edge, in a face: finite, and the face centres and edge midpoints of a cube give +-1/2-steps
    cu = Cs.model("cube")
    assert np.all(np.isfinite(cu.w))


@pytest.mark.parametrize("name", list(Cs.RECORDED))
def test_accuracy_against_brute_force(name):
    """The model against the plain sum with np.arctan2: the error at the default beta is no larger than recorded (x 1.5 for the
    last-bit differences of np.arctan2 between numpy builds); signs agree outside the margin; the margin is at most 2 % of the volume,
    and empty on watertight meshes."""
    rec = Cs.recorded()
    assert rec["default"] == Cs.DEFAULT_BETA and list(rec["betas"]) == list(Cs.BETAS)
    row = rec["cases"][name][repr(Cs.DEFAULT_BETA)]
    err, share = Cs.measure(name, Cs.DEFAULT_BETA)
    print(f"{name}: max |w_model - w_brute| = {err:.3e} (recorded {row['max_error']:.3e}), margin share {share:.4f}")
    assert err <= 1.5 * row["max_error"] + 4e-16
    wb = Cs.volume_brute(name)
    margin = np.abs(np.abs(wb) - 0.5) <= err
    assert margin.mean() <= 0.02
    if name not in Cs.OPEN:
        assert not margin.any()
    assert np.array_equal(Cs.volume_model(name).inside[~margin], (np.abs(wb) > 0.5)[~margin])


def test_default_beta_is_the_smallest_that_keeps_every_sign():
    rec = Cs.recorded()
    flips = {b: sum(rows[repr(b)]["sign_flips"] for rows in rec["cases"].values()) for b in rec["betas"]}
    assert flips[rec["default"]] == 0 and all(flips[b] > 0 for b in rec["betas"] if b < rec["default"]), flips
    from sdfkit_amd import meshsdf
    assert meshsdf.DEFAULT_WINDING_BETA == rec["default"]


def test_stated_atan2_is_accurate():
    rng = np.random.default_rng(5)
    y, x = rng.normal(size=20000), rng.normal(size=20000)
    assert np.abs(M.atan2_64(y, x) - np.arctan2(y, x)).max() < 1e-15
    e = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf])
    Y, X = np.meshgrid(e, e, indexing="ij")
    got, ref = M.atan2_64(Y, X), np.arctan2(Y, X)
    assert np.allclose(got, ref, atol=1e-15) and np.array_equal(np.signbit(got), np.signbit(ref))


def test_host_program_under_sanitizers(tmp_path):
    exe = Cs.build_host(tmp_path, sanitize=True)
    for name in ("degenerate", "two_cubes", "sphere_cap_removed", "bad_queries", "count_257"):
        c = Cs.case(name)
        h = Cs.host_run(exe, tmp_path, c["V"], c["T"], c["Q"], Cs.DEFAULT_BETA)
        same_answer(h, Cs.model(name))
        assert h.differs == 0
