"""The clouds of the orientation tests (tests/test_orient_model.py, tests/test_gpu_orient.py) with the side their normals should
point to, and the figures recorded in tests/golden/orient_cases.json.  Not a test module.

Every cloud is made from fixed seeds; normals come from tests/pointcloud_model.normals without a viewpoint -- the largest
component positive, so about half of them point inward on a closed surface."""
import numpy as np

from tests import orient_model as OM
from tests import pointcloud_model as PC

f32 = np.float32


def fibonacci(n, radius=1.0, centre=(0.0, 0.0, 0.0)):
    i = np.arange(n, dtype=np.float64) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    P = radius * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    return (P + np.asarray(centre, np.float64)).astype(f32)


def sphere():
    P = fibonacci(1000)
    return P, P.astype(np.float64)


def torus(n=3000, R=1.0, r=0.4):
    rs = np.random.default_rng(5)
    u, v = rs.random(n) * 2 * np.pi, rs.random(n) * 2 * np.pi
    out = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=1)
    P = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=1)
    return P.astype(f32), out


def clusters(count, n=400, gap=6.0):
    """`count` spheres far apart along x, each lower than the one before (so the seeds come in order)."""
    parts = [fibonacci(n, 1.0, (gap * c, 0.0, -0.25 * c)) for c in range(count)]
    out = [fibonacci(n).astype(np.float64) for _ in range(count)]
    return np.concatenate(parts).astype(f32), np.concatenate(out)


def box(half, n, seed):
    """n random points on the surface of the box [-half, half], uniform by area -> (points, the face normals)."""
    rs = np.random.default_rng(seed)
    h = np.asarray(half, np.float64)
    area = np.array([h[1] * h[2], h[0] * h[2], h[0] * h[1]])
    axis = rs.choice(3, n, p=area / area.sum())
    side = rs.choice([-1.0, 1.0], n)
    P = (rs.random((n, 3)) * 2 - 1) * h
    out = np.zeros((n, 3))
    P[np.arange(n), axis] = side * h[axis]
    out[np.arange(n), axis] = side
    return P.astype(f32), out


def cube():
    return box((1.0, 1.0, 1.0), 4000, 7)


def plate():
    return box((1.0, 1.0, 0.08), 4000, 8)


def strip(stations=400):
    """A helical strip two points wide: with k = 4 its graph is a ladder, and the rounds are about its length."""
    t = np.linspace(0.0, 6 * np.pi, stations)
    c = np.stack([np.cos(t), np.sin(t), 0.15 * t], axis=1)
    out = np.stack([np.cos(t), np.sin(t), np.zeros_like(t)], axis=1)
    P = np.stack([c - [0, 0, 0.02], c + [0, 0, 0.02]], axis=1).reshape(-1, 3)
    return P.astype(f32), np.repeat(out, 2, axis=0)


# name -> (cloud, k of the normals, k of the orientation, closed surface)
CASES = {
    "sphere": (sphere, 8, 8, True),
    "torus": (torus, 8, 8, True),
    "two_spheres": (lambda: clusters(2), 8, 8, True),
    "cube": (cube, 8, 8, True),
    "plate": (plate, 8, 8, True),
    "strip": (strip, 6, 4, False),
}
WITH_SINGLE_LEVEL = ("cube", "plate")

_made = {}


def cloud(name):
    """-> (points, outward directions, unoriented model normals), made once and read-only."""
    if name not in _made:
        make, kn = CASES[name][0], CASES[name][1]
        P, out = make()
        nrm, _ = PC.normals(P, kn)
        for a in (P, out, nrm):
            a.setflags(write=False)
        _made[name] = (P, out, nrm)
    return _made[name]


def fraction_right(normals, out, closed=True):
    """The fraction of normals on the side of `out`; an open surface has no outside: the better of the two."""
    f = float((np.einsum("ij,ij->i", np.asarray(normals, np.float64), out) > 0).mean())
    return f if closed else max(f, 1.0 - f)


def record(name, levels=OM.LEVELS):
    P, out, nrm = cloud(name)
    _, _, k, closed = CASES[name]
    got, st = OM.orient(P, nrm, k, levels=levels)
    return {"points": len(P), "k": k, "before": round(fraction_right(nrm, out, closed), 6), "after": round(fraction_right(got, out, closed), 6),
            "rounds": st["rounds"], "seeds": st["seeds"], "flipped": st["flipped"], "levels": st["levels"]}


def records():
    r = {name: record(name) for name in CASES}
    for name in WITH_SINGLE_LEVEL:
        r[name + "_single_level"] = record(name, levels=(0.0,))
    return r
