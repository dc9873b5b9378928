"""The clouds of the clustering tests (tests/test_points_cluster_model.py, tests/test_gpu_points_cluster.py), generated from seeds;
what the model gives on them is recorded in tests/golden/points_cluster_cases.json.  Not a test module."""
import json
import os

import numpy as np

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points_cluster_cases.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _sphere(rng, n, radius, centre):
    s = rng.standard_normal((n, 3))
    return s / np.linalg.norm(s, axis=1, keepdims=True) * radius + np.asarray(centre, np.float64)


def cloud_a(seed=7):
    """Three spheres of 1500, 700 and 300 points, radii 1, 0.5 and 0.25 around (0,0,0), (3,0,0) and (0,3,0), and 40 uniform strays in
    [-6, 6]^3, shuffled: -> (points (2540, 3) float32, which (2540,) int: the sphere 0 / 1 / 2 of a point, 3 for a stray)."""
    rng = np.random.default_rng(seed)
    parts = [_sphere(rng, 1500, 1.0, (0, 0, 0)), _sphere(rng, 700, 0.5, (3, 0, 0)), _sphere(rng, 300, 0.25, (0, 3, 0)), rng.uniform(-6, 6, (40, 3))]
    which = np.repeat(np.arange(4), [len(p) for p in parts])
    order = rng.permutation(len(which))
    return np.concatenate(parts)[order].astype(f32), which[order]


A_CASES = [(0.2, 1), (0.2, 6), (0.12, 10)]   # (radius, min_points)


def tie_clouds():
    """The tie of the border rule in its three index orders, from the golden file: -> [(name, points (9, 3) float32, labels, sizes)];
    min_points = 4, radius = 1: the origin is at distance exactly 1 from one core point of L and one of R."""
    t = golden()["tie"]
    return [(name, np.array(t["orders"][name]["points"], f32), t["orders"][name]["labels"], t["sizes"]) for name in ("L+R+origin", "R+L+origin", "origin+R+L")]


def chain(n=4096, seed=11):
    """n points at x = 0 .. n - 1, their indices shuffled: the deepest forest."""
    rng = np.random.default_rng(seed)
    P = np.zeros((n, 3), f32)
    P[:, 0] = rng.permutation(n)
    return P


BELOW_ONE = float(np.nextafter(f32(1), f32(0)))


def duplicates(seed=13):
    """5 points 3 times each and 4 distinct points, shuffled: (19, 3)."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, (9, 3)).astype(f32)
    P = np.concatenate([base[:5], base[:5], base[:5], base[5:]])
    return P[rng.permutation(len(P))]


def far_cloud(seed=17):
    """600 points of a sphere of radius 2 around 10^6 on every axis: the f32 spacing there is 0.0625, rounding makes duplicates."""
    rng = np.random.default_rng(seed)
    return _sphere(rng, 600, 2.0, (1e6, 1e6, 1e6)).astype(f32)


def two_sheets(seed=19, per=10_000):
    """2 x per points on z = 0 and z = 0.3 over [0, 4]^2, shuffled: -> (points, sheet (n,) int)."""
    rng = np.random.default_rng(seed)
    P = np.zeros((2 * per, 3))
    P[:, :2] = rng.uniform(0, 4, (2 * per, 2))
    sheet = np.repeat([0, 1], per)
    P[:, 2] = 0.3 * sheet
    order = rng.permutation(2 * per)
    return P[order].astype(f32), sheet[order]


SHEET_CASES = [(0.1, 1), (0.1, 8), (0.31, 8)]
