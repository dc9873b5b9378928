"""The triangle-mesh closest search and sign (csrc/lib_trimesh.hip: binning, the shell walk, its pruning bounds, ties, the column
items and crossing records) on the MI355X against the brute-force binary64 model (tests/meshsdf_model.py), bit for bit, on meshes
built to break a grid walk (tests/meshsdf_cases.py): mixed triangle sizes, flat and needle-shaped boxes, coordinates far from the
origin, two clusters with a void between them, exact ties across shells, nested shells, one triangle over every column.  Nothing
here has a tolerance: triangle index, f32 distance, closest point, voxel values and colours are compared as bits.

What fails when lib_trimesh.hip / trimesh_sdf.h is changed by one line (each built once, this module run once against it;
the same table is in DESIGN.md 8b):

1. if (lb > B.d2 || ...) break becomes lb >= B.d2
    not caught, and cannot be: it changes no result. The two differ only when lb == B.d2. For lb > 0 every unvisited
    triangle is strictly farther than lb (the gap had the slack taken off and the sum was scaled by 1 - 2^-18, more than its
    roundings), so none can tie with or beat B.d2. lb = 0 = B.d2 means the query lies on a triangle; a triangle at d2 = 0
    contains the query in its AABB, cell_of is monotone, so it is binned into the query's own cell and shell 0 has met every
    such triangle, the lowest index among them. lb = +inf only once every cell is visited.
2. the tie clause (C.d2 == B.d2 && (int)t < B.bi) removed
    caught: test_search_matches_brute_force[sheet, sheet100, tube, tie_shuffled, tie_appended, tie_prepended]
3. the x-face block skipped
    caught: 38 tests, among them test_search_matches_brute_force on 9 of its 10 meshes, test_volume_matches_model (20
    cases), all of test_band_against_unbanded_model, test_scans_of_more_than_one_block
4. - slack dropped from both shell gaps
    caught: test_search_needs_the_slack_of_its_shell_bound (added for it). The ten search meshes alone do not catch it, the
    far-offset ones included: at 65536 triangles, queries and the computed boundaries all sit on the same f32 lattice of
    1/128, so rounding never puts a triangle between a boundary and its computed position. The trap case finds, on the CPU
    restatement of the grid, coordinates just below a computed boundary that cell_of still puts into the upper cell, and
    places the closest triangle there and a slightly farther one in the query's own cell
5. stop2 replaced by band * band / 2
    caught: test_band_against_unbanded_model[mixed-1.0, mixed-20.0, clusters-20.0]
6. col_range's >= lo / <= hi made strict
    caught: test_nested_boxes_with_centres_on_faces, test_slab_columns_and_crossings[mesh_over_a_corner],
    test_volume_matches_model[far65536-ragged]; on the CPU test_col_range_matches_every_coordinate
"""
import functools

import numpy as np
import pytest

from sdfkit_amd import _native as N
from sdfkit_amd.meshsdf import MeshSdf
from tests import meshsdf_cases as Cs
from tests import meshsdf_model as M

pytestmark = pytest.mark.gpu
f32 = np.float32
f64 = np.float64

FAR = {"far4096": (4096.0, -8192.0, 1024.0), "far65536": (-65536.0, 3.0, 3.0)}


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "mixed":
        return Cs.mixed_sizes()
    if name == "mixed2400":
        return Cs.mixed_sizes(2400, seed=111)
    if name == "mixed_traps":
        return Cs.boundary_traps(*Cs.mixed_sizes())[:2]
    if name in FAR:
        V, T = Cs.mixed_sizes()
        return Cs.translated(V, FAR[name]), T
    if name == "sheet":
        return Cs.sheet()
    if name == "sheet100":
        return Cs.sheet(scale=(100.0, 1.0))
    if name == "tube":
        return Cs.tube()
    if name == "clusters":
        return Cs.two_clusters()
    if name.startswith("tie_"):
        return Cs.tie_lattice(name[4:])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def grid(name):
    return Cs.mesh_grid(*mesh(name))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _bits_equal(a, b, what=""):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.nonzero(_bits(a).reshape(-1) != _bits(b).reshape(-1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], a.reshape(-1)[bad[:5]], b.reshape(-1)[bad[:5]])


def _honest(name, t):
    """The conditions that keep a case from degenerating, on the CPU restatement of the grid and on the library's own figures."""
    V, T = mesh(name)
    G, s = grid(name), t.stats()
    assert tuple(s["grid"]) == G["dim"] and s["triangles"] == len(T) // 3, (name, s, G["dim"])
    assert s["entries"] == Cs.entries(G, V, T), (name, s)
    dim = G["dim"]
    if name in ("mixed", "mixed2400", "mixed_traps", "clusters") or name in FAR or name.startswith("tie_"):
        assert dim[0] * dim[1] * dim[2] >= 500, (name, dim)
    if name in ("sheet", "sheet100"):
        assert dim[2] == 1, (name, dim)
    if name == "tube":
        assert max(dim) >= 20 * min(dim), (name, dim)
    if name in ("mixed", "mixed2400"):
        assert s["entries"] > s["triangles"], (name, s)


# ---- Search -------------------------------------------------------------------------------------------------------------
NONFINITE = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf], [np.nan, np.nan, np.nan]], f32)


def _query_groups(name):
    V, T = mesh(name)
    g = {"random": Cs.random_queries(V, T, 260, 7), "surface": Cs.surface_queries(V, T, 130, 8), "outside": Cs.outside_queries(V, T)}
    if name == "clusters":
        g["void"] = Cs.cluster_queries()
    if name.startswith("tie_"):
        g["ties"] = Cs.tie_queries()
    return g


def _check_search(name, t, groups):
    V, T = mesh(name)
    keys = list(groups)
    Q = np.concatenate([groups[k] for k in keys] + [NONFINITE])
    tri, dist, cp = t.Search(Q)
    at = 0
    for k in keys:
        n = len(groups[k])
        rt, rd, rc, _, _ = M.closest(V, T, groups[k])
        got = tri[at:at + n]
        bad = np.nonzero(got != rt)[0]
        assert len(bad) == 0, (name, k, len(bad), bad[:5], got[bad[:5]], rt[bad[:5]], dist[at:at + n][bad[:5]], rd[bad[:5]])
        _bits_equal(dist[at:at + n], rd, (name, k, "distance"))
        _bits_equal(cp[at:at + n], rc, (name, k, "closest point"))
        at += n
    assert np.all(tri[at:] == -1) and np.all(np.isposinf(dist[at:])) and np.all(np.isnan(cp[at:]))


SEARCH_MESHES = ["mixed", "sheet", "sheet100", "tube", "far4096", "far65536", "clusters", "tie_shuffled", "tie_appended", "tie_prepended"]


@pytest.mark.parametrize("name", SEARCH_MESHES)
def test_search_matches_brute_force(gpu, name):
    """Random points in the box enlarged by 50 %, mesh vertices and edge midpoints, and the outside list (axes and corner
    directions at 10, 1000 and 10^6 extents; the box's corners and face centres); non-finite queries give (-1, +inf, NaN)."""
    t = MeshSdf(mesh(name))
    _honest(name, t)
    _check_search(name, t, _query_groups(name))


@pytest.mark.parametrize("variant", ["shuffled", "appended", "prepended"])
def test_tie_cases_do_tie_across_cells(variant):
    """On the model alone (no device): the tie queries really have several triangles at exactly the least d2, with the winner in
    another cell row than the runner-up, and first met in a later shell than another triangle at that distance."""
    name = "tie_" + variant
    V, T = mesh(name)
    tied, other_row, later_shell = Cs.tie_statistics(V, T, Cs.tie_queries(), grid(name))
    assert tied >= 100 and other_row >= 20 and later_shell >= 20, (tied, other_row, later_shell)


def test_search_needs_the_slack_of_its_shell_bound(gpu):
    """Queries a few thousandths of a cell below a cell boundary whose f32 position in the shell bound lies above coordinates that
    cell_of puts into the upper cell: the closest triangle is binned there only, and a triangle in the query's own cell is
    nearer than the bound of shell 0 computed without slack.  Both are asserted on the CPU; the device must still answer exactly."""
    name = "mixed_traps"
    V, T = mesh(name)
    _, _, Q, winners = Cs.boundary_traps(*Cs.mixed_sizes())
    assert len(Q) >= 8 and grid(name)["dim"] == grid("mixed")["dim"]
    rt, _, _, _, _ = M.closest(V, T, Q)
    assert np.array_equal(rt, winners)
    for q, w in zip(Q, winners):
        stops, own_best = Cs.stops_early_without_slack(grid(name), V, T, q)
        assert stops and own_best != w, (q, w, own_best)
    t = MeshSdf((V, T))
    _honest(name, t)
    _check_search(name, t, {"traps": Q, "random": Cs.random_queries(V, T, 100, 9)})


def test_search_prunes_while_exact(gpu):
    """With profiling on, the mixed-size mesh: far fewer closest-point evaluations per query than triangles, same results."""
    V, T = mesh("mixed")
    t = MeshSdf((V, T))
    Q = Cs.random_queries(V, T, 260, 7)
    N.check(N.lib().sdfk_profile_enable(1))
    try:
        tri, dist, cp = t.Search(Q)
        s = t.stats()
    finally:
        N.check(N.lib().sdfk_profile_enable(0))
    assert s["queries"] == len(Q) and s["candidates"] >= len(Q), s
    print("candidates per query", s["candidates"] / s["queries"], "triangles", s["triangles"])
    assert s["candidates"] / s["queries"] < s["triangles"] / 4, s
    rt, rd, rc, _, _ = M.closest(V, T, Q)
    assert np.array_equal(tri, rt)
    _bits_equal(dist, rd)
    _bits_equal(cp, rc)


# ---- ToVoxels -----------------------------------------------------------------------------------------------------------
def _wide_box(name, k):
    """The mesh's box enlarged to k times its extent about its centre (an axis of no extent: as the largest one), as f32."""
    lo, hi = Cs.box_of(*mesh(name))
    c, e = 0.5 * (lo + hi), hi - lo
    e = np.where(e > 0, e, e.max())
    return (c - 0.5 * k * e).astype(f32), (c + 0.5 * k * e).astype(f32)


def _volume_spec(name, kind):
    lo, hi = Cs.box_of(*mesh(name))
    e = np.where(hi - lo > 0, hi - lo, (hi - lo).max())
    if kind == "outside":      # wholly outside the mesh's box, off its (+, +, +) corner
        return (hi + 0.5 * e).astype(f32), (hi + 1.5 * e).astype(f32), (9, 8, 7)
    if kind == "one_cell":     # wholly inside one cell of the search grid
        G = grid(name)
        c = np.array(G["dim"]) // 2
        o = G["lo"].astype(f64) + c * f64(G["h"])
        return (o + 0.2 * f64(G["h"])).astype(f32), (o + 0.8 * f64(G["h"])).astype(f32), (7, 6, 5)
    mn, mx = _wide_box(name, 1.3)
    return mn, mx, {"ragged": (24, 20, 18), "ny1": (17, 1, 29), "nx1": (1, 19, 23), "nz1": (21, 16, 1)}[kind]


def _sample(n, k, seed):
    total = n[0] * n[1] * n[2]
    if total <= k:
        return np.stack([a.reshape(-1) for a in np.meshgrid(*[np.arange(m) for m in n], indexing="ij")], 1)
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, n[a], k) for a in range(3)], 1)


def _check_volume(name, t, mn, mx, n, idx, colors=None):
    V, T = mesh(name)
    vox = t.ToVoxels(list(mn), list(mx), *n)
    vals, cols = M.volume(V, T, mn, mx, n, colors=colors, sample=idx)
    _bits_equal(vox.Values[idx[:, 0], idx[:, 1], idx[:, 2]], vals, (name, n, "values"))
    if colors is not None:
        _bits_equal(vox.Colors[idx[:, 0], idx[:, 1], idx[:, 2]], cols, (name, n, "colours"))
    return vals


VOLUME_MESHES = ["mixed", "sheet", "far4096", "far65536", "clusters"]


@pytest.mark.parametrize("kind", ["ragged", "ny1", "nx1", "nz1", "outside", "one_cell"])
@pytest.mark.parametrize("name", VOLUME_MESHES)
def test_volume_matches_model(gpu, name, kind):
    mn, mx, n = _volume_spec(name, kind)
    d, m = M.grid_constants(mn, mx, n)
    centres = np.stack([M.coord(m[a], np.array([0, n[a] - 1]), d[a]) for a in range(3)], 1)   # the two extreme centres
    if kind == "one_cell":
        cells = Cs.cell_of(grid(name), centres)
        assert np.all(cells[0] == cells[1]) and np.all(cells[0] == np.array(grid(name)["dim"]) // 2), cells
    if kind == "outside":
        assert np.all(centres[0] > Cs.box_of(*mesh(name))[1])
    t = MeshSdf(mesh(name))
    vals = _check_volume(name, t, mn, mx, n, _sample(n, 300, 31))
    assert np.all(np.isfinite(vals))


def test_volume_with_colours(gpu):
    V, T = mesh("mixed")
    colors = np.random.default_rng(41).uniform(0.05, 1.0, V.shape).astype(f32)
    mn, mx, n = _volume_spec("mixed", "ragged")
    _check_volume("mixed", MeshSdf((V, T, colors)), mn, mx, n, _sample(n, 300, 32), colors=colors)


# ---- Band ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [0.25, 1.0, 20.0])
@pytest.mark.parametrize("name", ["mixed", "clusters"])
def test_band_against_unbanded_model(gpu, name, cells):
    """A band of a quarter of a cell edge, one cell edge and 20 cell edges: voxels the unbanded model has within the band keep
    the model's bits, every other voxel is exactly +-band with the model's sign.  Half of the sampled voxels are those of mesh
    vertices, the others anywhere in a volume that reaches 1.5 bands beyond the mesh."""
    V, T = mesh(name)
    band = f32(cells * f64(grid(name)["h"]))
    lo, hi = Cs.box_of(V, T)
    reach = 1.5 * f64(band) + 0.05 * (hi - lo).max()
    mn, mx = (lo - reach).astype(f32), (hi + reach).astype(f32)
    step = max(f64(band) / 2, (mx - mn).max() / 320.0)
    n = tuple(int(min(max(np.ceil((mx[a] - mn[a]) / step), 6), 320)) + a for a in range(3))
    d, m = M.grid_constants(mn, mx, n)
    rng = np.random.default_rng(51)
    near = V[rng.integers(0, len(V), 300)]
    near = np.stack([np.clip(np.floor((near[:, a].astype(f64) - f64(m[a])) / f64(d[a]) + 0.5), 0, n[a] - 1) for a in range(3)], 1).astype(np.int64)
    idx = np.concatenate([near, _sample(n, 300, 52)])
    model, _ = M.volume(V, T, mn, mx, n, sample=idx)
    got = MeshSdf((V, T)).ToVoxels(list(mn), list(mx), *n, maxDistance=band).Values[idx[:, 0], idx[:, 1], idx[:, 2]]
    inb = np.abs(model) <= band
    print(name, cells, "band", band, "n", n, "in band", np.count_nonzero(inb), "of", len(inb))
    assert np.count_nonzero(inb) >= 10 and np.count_nonzero(~inb) >= 10, (np.count_nonzero(inb), len(inb))
    _bits_equal(got[inb], model[inb], (name, cells, "in band"))
    assert np.all(np.abs(got[~inb]) == band), (name, cells, got[~inb][np.abs(got[~inb]) != band][:5])
    assert np.array_equal(np.signbit(got[~inb]), np.signbit(model[~inb]))


# ---- Sign ---------------------------------------------------------------------------------------------------------------
def _centres(mn, mx, n):
    d, m = M.grid_constants(mn, mx, n)
    return [M.coord(m[a], np.arange(n[a]), d[a]) for a in range(3)]


def _full_volume(V, T, mn, mx, n, t=None):
    t = t or MeshSdf((V, T))
    got = t.ToVoxels(list(mn), list(mx), *n).Values
    vals, _ = M.volume(V, T, mn, mx, n)
    _bits_equal(got, vals)
    return t, vals


def _model_crossings(V, T, mn, mx, n):
    d, m = M.grid_constants(mn, mx, n)
    return len(M.crossings(V, T, m, d, n[0], n[1])[0])


def test_nested_boxes_sign_is_parity_of_containment(gpu):
    """12 concentric closed boxes, no voxel centre on a face: the model's bits, and negative exactly where the number of boxes
    that contain the centre is odd."""
    halves = np.array([(0.06 + 0.072 * k) * np.array([1.0, 0.9, 0.8]) for k in range(12)], f32)
    V, T = Cs.nested_boxes(halves)
    mn, mx, n = [-1.0] * 3, [1.0] * 3, (24, 20, 18)
    xs = _centres(mn, mx, n)
    for a in range(3):
        assert not np.any(np.abs(xs[a])[:, None] == halves[None, :, a]), a
    t, vals = _full_volume(V, T, mn, mx, n)
    X = np.meshgrid(*xs, indexing="ij")
    inside = np.zeros(n, np.int64)
    for h in halves:
        inside += (np.abs(X[0]) < h[0]) & (np.abs(X[1]) < h[1]) & (np.abs(X[2]) < h[2])
    assert np.array_equal(vals < 0, inside % 2 == 1) and np.all(vals != 0)
    assert len(np.unique(inside)) >= 6   # (the grid resolves several levels of nesting)
    assert t.stats()["crossings"] == _model_crossings(V, T, mn, mx, n)


def test_nested_boxes_with_centres_on_faces(gpu):
    """12 nested boxes whose faces lie exactly on voxel-centre coordinates (columns on the edges of the triangles' boxes): against
    the model only -- on a face the sign follows the perturbation rule, not an analytic one."""
    mn, mx, n = [-1.0] * 3, [1.0] * 3, (26, 26, 26)
    xs = _centres(mn, mx, n)
    los = [[xs[a][12 - k] for a in range(3)] for k in range(12)]
    his = [[xs[a][13 + k] for a in range(3)] for k in range(12)]
    V, T = Cs.nested_boxes_between(los, his)
    t, vals = _full_volume(V, T, mn, mx, n)
    assert np.count_nonzero(vals == 0) > 1000   # (centres on faces)
    assert t.stats()["crossings"] == _model_crossings(V, T, mn, mx, n)


SLABS = {
    # mesh box, volume min, max, n
    "over_every_column": (([-2.0, -1.6, -0.1], [2.0, 1.6, 0.1]), [-1.5, -1.2, -0.4], [1.5, 1.2, 0.4], (96, 80, 5)),
    "mesh_much_larger": (([-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]), [0.31, -0.05, 0.2], [0.41, 0.05, 0.3], (12, 10, 9)),
    "mesh_over_a_corner": (([0.5, 0.5, -0.2], [0.9, 0.9, 0.2]), [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], (20, 18, 10)),
}


@pytest.mark.parametrize("case", list(SLABS))
def test_slab_columns_and_crossings(gpu, case):
    """A closed slab (two horizontal quads joined by side walls): its four horizontal triangles each span every column of the
    volume, or the mesh dwarfs the volume, or covers a corner of it.  Values against the model; the crossing records counted."""
    box, mn, mx, n = SLABS[case]
    V, T = M.box_mesh(*box)
    t, vals = _full_volume(V, T, mn, mx, n)
    s = t.stats()
    want = _model_crossings(V, T, mn, mx, n)
    assert s["crossings"] == want, (s, want)
    xs = _centres(mn, mx, n)
    covered = np.count_nonzero((xs[0] >= f32(box[0][0])) & (xs[0] < f32(box[1][0]))) * np.count_nonzero((xs[1] >= f32(box[0][1])) & (xs[1] < f32(box[1][1])))
    assert want == 2 * covered > 0   # (every covered column crosses the bottom and the top once)
    if case == "over_every_column":
        assert covered == n[0] * n[1] and s["entries"] > s["triangles"], s
        assert np.array_equal(vals < 0, np.broadcast_to(np.abs(xs[2]) < f32(0.1), n))
    if case == "mesh_much_larger":
        assert np.all(vals < 0)


def test_vertical_triangles_cross_nothing(gpu):
    """Only the side walls of a box (zero projected area): no crossing record, no negative value."""
    V, T = M.box_mesh([-0.5, -0.4, -0.3], [0.5, 0.4, 0.3])
    T = T[12:]
    P = V[T.reshape(-1, 3)]
    assert np.all(M.orient2d_exact(P[:, 0, 0], P[:, 0, 1], P[:, 1, 0], P[:, 1, 1], P[:, 2, 0], P[:, 2, 1]) == 0)
    mn, mx, n = [-1.0] * 3, [1.0] * 3, (16, 14, 12)
    t, vals = _full_volume(V, T, mn, mx, n)
    assert t.stats()["crossings"] == 0 and np.all(vals >= 0) and not np.any(np.signbit(vals))


# ---- Scan regimes -------------------------------------------------------------------------------------------------------
def test_scans_of_more_than_one_block(gpu):
    """More than 2048 triangles, cells and columns: the item scan, the column scan and the cell scans (csrc/device_scan.h, 2048
    values per block) all take more than one block."""
    name = "mixed2400"
    V, T = mesh(name)
    t = MeshSdf((V, T))
    _honest(name, t)
    mn, mx = _wide_box(name, 1.1)
    n = (64, 40, 5)
    s = t.stats()
    assert s["triangles"] > 2048 and s["grid"][0] * s["grid"][1] * s["grid"][2] > 2048 and n[0] * n[1] > 2048
    _check_volume(name, t, mn, mx, n, _sample(n, 1000, 61))
    assert t.stats()["crossings"] == _model_crossings(V, T, mn, mx, n) > 2048
