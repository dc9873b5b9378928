"""Degenerate neighbourhoods and sparse volumes for point-cloud normals and volumes (csrc/points_normals.h, csrc/lib_pointcloud.hip;
tests/test_pointcloud_cases.py on the CPU, tests/test_gpu_pointcloud_stress.py on the MI355X): deterministic generators with fixed
seeds, float32 out.  Not a test module.

clusters(): 64 points per cluster about centres on a lattice 8 apart, offsets of at most about 0.5 -- so for k <= 64 the neighbours
of a point are points of its own cluster, while the search still decides their order and breaks their ties.  The offsets of the
families called exact are small dyadic numbers (multiples of 2^-10 below 1), so that centre + offset, the differences of two
points and the d2 of the search are all exact in float32: "on a plane" and "on a line" hold without rounding.
"""
import numpy as np

from tests import points_cases as PCS

f32, f64 = np.float32, np.float64

POINTS_PER_CLUSTER = 64
CLUSTERS_PER_FAMILY = 4
SPACING = 8.0
# family label -> name, in the order of the clusters
FAMILIES = ("generic", "near_planar", "planar_tilted", "collinear_x", "collinear_tilted", "sphere", "lattice", "copies", "copies_rank1",
            "copies_rank2", "two_points", "needle", "plane_xy")
FAMILY = {name: i for i, name in enumerate(FAMILIES)}
# what the families promise, for the tests that derive their expectations from the labels
PLANE_DIRECTIONS = {"planar_tilted": ((1.0, 0.5, 0.25), (0.0, 1.0, -0.5)), "plane_xy": ((1.0, -1.0, 0.0), (0.0, 0.0, 1.0))}
LINE_DIRECTIONS = {"collinear_x": (1.0, 0.0, 0.0), "collinear_tilted": (1.0, -0.5, 0.75)}
# how many of a cluster's 64 points sit on one position (the rest are distinct from it and from each other) ...
COPIES = {"copies": 64, "copies_rank1": 63, "copies_rank2": 62, "two_points": 32}
# ... and the lattice family: its 27 positions twice, the first ten a third time
LATTICE_TRIPLES = 10


def _dyadic(x, bits=10):
    return np.round(np.asarray(x, f64) * 2.0 ** bits) / 2.0 ** bits


def _distinct(rng, n, span, bits):
    """n distinct multiples of 2^-bits in [-span, span]."""
    m = int(span * 2 ** bits)
    return rng.choice(np.arange(-m, m + 1), n, replace=False) / 2.0 ** bits


def _offsets(rng, family):
    n = POINTS_PER_CLUSTER
    g = _dyadic(np.clip(rng.normal(0.0, 0.15, (n, 3)), -0.5, 0.5))
    name = FAMILIES[family]
    if name == "generic":
        return g
    if name == "near_planar":
        g[:, 2] *= 2.0 ** -10
        return g
    if name == "planar_tilted":                    # a (1, 1/2, 1/4) + b (0, 1, -1/2)
        a, b = _dyadic(np.clip(rng.normal(0.0, 0.1, (2, n)), -0.25, 0.25), 8)
        return np.stack([a, a / 2 + b, a / 4 - b / 2], axis=1)
    if name == "collinear_x":
        return np.stack([_distinct(rng, n, 0.5, 9), np.zeros(n), np.zeros(n)], axis=1)
    if name == "collinear_tilted":                 # t (1, -1/2, 3/4)
        t = _distinct(rng, n, 0.375, 8)
        return np.stack([t, -t / 2, 3 * t / 4], axis=1)
    if name == "sphere":
        d = rng.normal(size=(n, 3))
        return _dyadic(0.25 * d / np.linalg.norm(d, axis=1, keepdims=True))
    if name == "lattice":                          # {-1/8, 0, 1/8}^3: positions 0 .. 26 twice, 0 .. 9 three times
        p = np.arange(n) % 27
        return (np.stack([p // 9, (p // 3) % 3, p % 3], axis=1) - 1) / 8.0
    if name == "copies":
        return np.zeros((n, 3))
    if name == "copies_rank1":
        off = np.zeros((n, 3))
        off[0] = _dyadic(rng.uniform(0.125, 0.5, 3) * rng.choice([-1, 1], 3))
        return off
    if name == "copies_rank2":
        off = np.zeros((n, 3))
        off[0] = _dyadic(rng.uniform(0.125, 0.5, 3) * rng.choice([-1, 1], 3))
        off[1] = off[0][[1, 2, 0]] * [1, -1, 1]    # not on the line through off[0] and the copies
        assert np.linalg.norm(np.cross(off[0], off[1])) > 0
        return off
    if name == "two_points":
        off = np.zeros((n, 3))
        off[::2] = _dyadic(rng.uniform(0.125, 0.5, 3) * rng.choice([-1, 1], 3))
        return off
    if name == "needle":
        g[:, 0] = _distinct(rng, n, 0.5, 9)
        g[:, 1:] *= 2.0 ** -20
        return g
    if name == "plane_xy":                         # x + y constant: (a, -a, b)
        a, b = _dyadic(np.clip(rng.normal(0.0, 0.1, (2, n)), -0.25, 0.25), 8)
        return np.stack([a, -a, b], axis=1)
    raise KeyError(name)


_made = {}


def clusters(seed):
    """-> (points (n, 3) float32, family (n,) int64), n = 13 families x 4 clusters x 64 points, in a random order (so that the
    index, which breaks the ties of the search, says nothing about the cluster).  Read-only, made once per seed."""
    if seed not in _made:
        rng = np.random.default_rng(seed)
        pts, fam = [], []
        for family in range(len(FAMILIES)):
            for r in range(CLUSTERS_PER_FAMILY):
                c = family * CLUSTERS_PER_FAMILY + r
                centre = SPACING * np.array([c % 4, (c // 4) % 4, c // 16], f64)
                pts.append(centre[None, :] + _offsets(rng, family))
                fam.append(np.full(POINTS_PER_CLUSTER, family))
        order = rng.permutation(len(FAMILIES) * CLUSTERS_PER_FAMILY * POINTS_PER_CLUSTER)
        P = np.ascontiguousarray(np.concatenate(pts)[order].astype(f32))
        F = np.concatenate(fam)[order].astype(np.int64)
        P.setflags(write=False)
        F.setflags(write=False)
        _made[seed] = (P, F)
    return _made[seed]


def cluster_centre(family, r):
    """The centre of cluster r (0 .. 3) of a family."""
    c = FAMILY[family] * CLUSTERS_PER_FAMILY + r
    return SPACING * np.array([c % 4, (c // 4) % 4, c // 16], f64)


SCALES = (-70, 40, -140)


def scaled_clusters(seed, e):
    """clusters(seed) times 2^e.  e = -70: the d2 within a cluster are subnormal float32 (or 0); +40: large but finite; -140: the
    coordinates are subnormal themselves and every d2 is 0, so the index alone orders the neighbours."""
    P, F = clusters(seed)
    S = PCS.scaled(P, e)
    S.setflags(write=False)
    return S, F


def multiplicity(P):
    """Per point, how many points of P sit on its position (itself included)."""
    _, inverse, counts = np.unique(np.asarray(P), axis=0, return_inverse=True, return_counts=True)
    return counts[inverse.reshape(-1)]


def hand_made_neighbourhoods():
    """Neighbourhoods with exact ties that a random cluster need not hold -> (centre (c, 3), neighbours (c, 64, 3), m (c,)) float32 /
    int32, the point first among its neighbours, in the layout tests/cpp/points_normals_host.cpp reads."""
    rows = []

    def add(centre, offsets):
        nb = np.zeros((64, 3))
        nb[:len(offsets)] = np.asarray(centre, f64)[None] + np.asarray(offsets, f64)
        rows.append((np.asarray(centre, f64), nb, len(offsets)))

    e = np.eye(3)
    octa = np.concatenate([np.zeros((1, 3)), 0.25 * e, -0.25 * e])
    add((1, 2, 3), octa)                                            # three equal eigenvalues, a diagonal covariance
    add((1, 2, 3), octa * [1, 1, 0.5])                              # l_2 least
    add((1, 2, 3), octa * [0.5, 1, 0.5])                            # l_0 == l_2 least: the lower column
    add((1, 2, 3), octa * [1, 0.5, 0.5])                            # l_1 == l_2 least
    add((-4, 0, 8), octa * [0.5, 0.5, 1])                           # l_0 == l_1 least
    sq = np.array([[0, 0, 0], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0]]) / 8.0
    add((0, 0, 0), sq)                                              # a square in z = 0
    add((2, 2, 2), sq[:, [0, 2, 1]])                                # ... in y = 0
    add((2, 2, 2), sq[:, [2, 0, 1]])                                # ... in x = 0
    diag = np.array([[0, 0, 0], [1, -1, 0], [-1, 1, 0], [0, 0, 1], [0, 0, -1], [1, -1, 1], [-1, 1, -1]]) / 8.0
    add((5, -3, 1), diag)                                           # the plane x + y = const: c00 == c11, theta == 0
    add((5, -3, 1), diag[:, [2, 0, 1]])                             # y + z = const
    add((5, -3, 1), diag[:, [0, 2, 1]])                             # x + z = const
    add((5, -3, 1), -diag[:, [0, 2, 1]] * [1, -1, 1])               # x - z = const
    add((0, 0, 0), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]]) / 4.0)       # m = 3
    add((0, 0, 0), np.array([[0, 0, 0], [1, 0, 0]]) / 4.0)                  # m = 2: degenerate
    add((7, 7, 7), np.zeros((5, 3)))                                        # trace 0
    centre = np.array([r[0] for r in rows]).astype(f32)
    nb = np.array([r[1] for r in rows]).astype(f32)
    return centre, nb, np.array([r[2] for r in rows], np.int32)


# ---- volumes ----
def sparse_normal_cloud(seed):
    """300 points uniform in the unit cube with random unit normals, about half of which are (0, 0, 0) in either sign of zero: a
    cloud that, sampled with a band, leaves most lines and whole slabs of a volume without a sign.  No point within 0.1 of the line
    y = z = 0.5 has a normal, so a volume of one line of cells along x through the middle of BOX, sampled with a band below 0.1, has
    no known voxel at all.  -> (points, normals) float32."""
    rng = np.random.default_rng(seed)
    P = rng.random((300, 3), dtype=f32)
    Nn = rng.normal(size=(300, 3))
    Nn = (Nn / np.linalg.norm(Nn, axis=1, keepdims=True)).astype(f32)
    none = (rng.random(300) < 0.5) | (np.hypot(P[:, 1].astype(f64) - 0.5, P[:, 2].astype(f64) - 0.5) <= 0.1)
    Nn[none] = np.where(rng.random((int(none.sum()), 3)) < 0.5, f32(-0.0), f32(0.0))
    return np.ascontiguousarray(P), np.ascontiguousarray(Nn)


BOX = ((-0.5, -0.5, -0.5), (1.5, 1.5, 1.5))
# thickness 1 along one axis, along two, a small odd volume, and one with more than 256 lines in each pass of the fill, none a
# multiple of 256 (19 * 18 = 342, 19 * 15 = 285, 18 * 15 = 270)
VOLUME_SHAPES = ((1, 1, 37), (1, 19, 1), (23, 1, 1), (9, 7, 1), (5, 1, 11), (13, 11, 9), (19, 18, 15))
K_AND_BAND = ((1, np.inf), (1, 0.08), (8, 0.08), (64, 0.3))
SHAPES = [(shape, k, md) for shape in VOLUME_SHAPES for k, md in K_AND_BAND]


# ---- volumes over the clusters ----
# 16^3 cells of edge 1 whose centres are the integers 4 .. 19, 16 .. 31, 0 .. 15: eight clusters lie inside, and the cell centres
# (8, 24, 8) and (16, 24, 8) are exactly the positions of two clusters of 64 copies
CLUSTER_BOX = ((3.5, 15.5, -0.5), (19.5, 31.5, 15.5))
CLUSTER_SHAPE = (16, 16, 16)
COPIES_VOXELS = ((4, 8, 8), (12, 8, 8))


def cluster_normals(seed):
    """One normal per point of clusters(seed): random unit vectors, 30 % of them (0, 0, 0) -- but the lowest-numbered copy of each
    cluster of copies keeps one, so that the nearest point (k = 1) of a query at the copies speaks."""
    P, F = clusters(seed)
    rng = np.random.default_rng(seed + 1000)
    Nn = rng.normal(size=P.shape)
    Nn = (Nn / np.linalg.norm(Nn, axis=1, keepdims=True)).astype(f32)
    none = rng.random(len(P)) < 0.3
    copies = np.flatnonzero(F == FAMILY["copies"])
    _, first = np.unique(P[copies], axis=0, return_index=True)     # (flatnonzero ascends: the first of a position is its lowest index)
    none[copies[first]] = False
    Nn[none] = 0
    return np.ascontiguousarray(Nn)
