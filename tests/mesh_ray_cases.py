"""The cases of the mesh ray tests (tests/test_mesh_ray_host.py on the CPU, tests/test_gpu_mesh_ray.py on the device): the smallest
shapes at which the grid walk of csrc/trimesh_ray.h can still go wrong.  A case is a dict: V (nv, 3) f32, T (nt, 3) int32, colors or
None, O / D (n, 3) f32 rays, tmin, tmax.  RENDER holds the camera cases.  Everything is deterministic; the marching-cubes spheres
come from the CPU reference (oracle), whose meshes the library reproduces bit for bit, and are made once."""
import functools

import numpy as np

from tests import meshsdf_cases as G

f32, f64, i32 = np.float32, np.float64, np.int32
INF = np.inf


def _case(V, T, O, D, tmin=0.0, tmax=INF, colors=None):
    O, D = np.ascontiguousarray(np.asarray(O, f32).reshape(-1, 3)), np.ascontiguousarray(np.asarray(D, f32).reshape(-1, 3))
    assert O.shape == D.shape
    return {"V": np.ascontiguousarray(np.asarray(V, f32).reshape(-1, 3)), "T": np.ascontiguousarray(np.asarray(T, i32).reshape(-1, 3)),
            "colors": colors, "O": O, "D": D, "tmin": float(tmin), "tmax": float(tmax)}


def aimed(origin, targets):
    """rays from one origin (or one per target) at the targets: d = f32(target - origin)"""
    P = np.asarray(targets, f32).reshape(-1, 3)
    O = np.broadcast_to(np.asarray(origin, f32).reshape(-1, 3), P.shape).copy()
    return O, (P - O).astype(f32)


def directions(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def position_colors(V):
    """vertex colours that are a fixed f32 function of the position, never all zero"""
    V = np.asarray(V, f32).reshape(-1, 3)
    return np.ascontiguousarray((f32(0.25) + f32(0.5) * np.abs(np.sin(V * f32(3.0)))).astype(f32))


def edges_of(T):
    T = np.asarray(T, np.int64).reshape(-1, 3)
    e = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])
    return np.unique(np.sort(e, 1), axis=0)


# ---- meshes ----------------------------------------------------------------------------------------------------------------------
def cube(lo=0.0, hi=1.0):
    c = np.array([[x, y, z] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], f32)
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    T = np.array([t for a, b, cc, d in q for t in ((a, b, cc), (a, cc, d))], i32)
    return c, T


@functools.lru_cache(maxsize=None)
def mc_sphere(n, radius=1.0, half=1.25):
    from oracle import oracle as O
    s = O.Scene()
    s.sphere_w(radius)
    mn, mx = [-half] * 3, [half] * 3
    vals, _ = O.sample(s, mn, mx, n, n, n, with_colors=False)
    m = O.march(vals, None, mn, mx)
    V, T = np.ascontiguousarray(m.vertices, f32), np.ascontiguousarray(m.triangles.reshape(-1, 3), i32)
    V.setflags(write=False)
    T.setflags(write=False)
    return V, T


def fillers(n, lo, hi, size, seed, avoid=None):
    """n small triangles scattered in the box (they size the grid), none within `avoid` = (point, direction, radius) of a line"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, f64), np.asarray(hi, f64)
    out = []
    while len(out) < n:
        c = rng.uniform(lo, hi)
        if avoid is not None:
            p, d, r = avoid
            d = np.asarray(d, f64) / np.linalg.norm(d)
            w = c - np.asarray(p, f64)
            if np.linalg.norm(w - d * (w @ d)) < r:
                continue
        out.append(np.clip(c + rng.uniform(-size, size, (3, 3)), lo, hi))
    return G.soup(np.array(out))


# ---- the hand-made cases ---------------------------------------------------------------------------------------------------------
def single_triangle():
    V, T = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], f32), np.array([(0, 1, 2)], i32)
    pts = [(0.25, 0.25), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]
    up, dn = np.nextafter(f32(0), f32(1)), np.nextafter(f32(0), f32(-1))
    pts += [(0.5, dn), (dn, 0.5), (np.nextafter(f32(0.5), f32(1)), 0.5), (dn, dn), (np.nextafter(f32(1), f32(2)), 0.0), (0.0, np.nextafter(f32(1), f32(2))),
            (0.5, up), (up, 0.5), (np.nextafter(f32(0.5), f32(0)), 0.5)]
    O, D = [], []
    for x, y in pts:
        for z, dz in ((1.0, -1.0), (-1.0, 1.0), (0.5, -2.0)):
            O.append((x, y, z)); D.append((0.0, 0.0, dz))
        # slanted: aimed at the same point from off-axis origins on both sides
        for o in ((0.7, -0.4, 1.3), (-0.6, 0.9, -0.8)):
            O.append(o); D.append(tuple(np.asarray((x, y, 0.0), f32) - np.asarray(o, f32)))
    # parallel to the plane, and in the plane (det == 0)
    for o, d in (((-1, 0.25, 0.5), (1, 0, 0)), ((-1, 0.25, 0.0), (1, 0, 0)), ((0.25, -1, 0.0), (0, 1, 0)), ((2, 2, 0.0), (-1, -1, 0)),
                 ((0.25, 0.25, 0.0), (1, 0, 0)), ((-1, 0.25, 0.0), (-1, 0, 0))):
        O.append(o); D.append(d)
    return _case(V, T, O, D, -INF, INF)


def _patch():
    """2 x 2 unit quads over [0, 2]^2 in z = 0, each split along its (0, 0)-(1, 1) diagonal: the vertex (1, 1) and the edges that
    meet in it are interior, so the watertight test lets no ray aimed at them through"""
    V = np.array([(x, y, 0) for y in range(3) for x in range(3)], f32)
    T = []
    for j in range(2):
        for i in range(2):
            a = 3 * j + i
            T += [(a, a + 1, a + 4), (a, a + 4, a + 3)]
    return V, np.array(T, i32)


def _edge_rays():
    """at points of the interior shared edges and at the shared interior vertex: perpendicular from both sides (exact: a true
    tie, which the lowest index wins) and slanted from three origins (rounded directions: some neighbour is hit)"""
    pts = [(k / 8.0, k / 8.0, 0.0) for k in range(1, 16)] + [(1.0, k / 8.0, 0.0) for k in range(1, 16)] + [(k / 8.0, 1.0, 0.0) for k in range(1, 16)] + \
        [(1 / 3.0, 1 / 3.0, 0.0), (1.7, 1.7, 0.0), (1.0, 0.3, 0.0)]
    O, D = [], []
    for p in pts:
        p = np.asarray(p, f32)
        for o in ((0.2, 0.9, 1.5), (0.875, 0.125, -2.0), (p[0], p[1], 1.0), (p[0], p[1], -1.0), (3.0, -2.0, 0.25)):
            O.append(o); D.append(tuple(p - np.asarray(o, f32)))
    return O, D


def lowest_containing(V, T, O):
    """for rays perpendicular to the plane z = 0 through (O.x, O.y): the lowest index of a triangle whose closed area holds the point
    (float64 from the f32 inputs; exact for the dyadic coordinates of the patch), -1: none"""
    V, T = np.asarray(V, f64), np.asarray(T, np.int64).reshape(-1, 3)
    out = np.full(len(O), -1, np.int64)
    for r, o in enumerate(np.asarray(O, f64)):
        for t in range(len(T) - 1, -1, -1):
            a, b, c = V[T[t, 0], :2] - o[:2], V[T[t, 1], :2] - o[:2], V[T[t, 2], :2] - o[:2]
            u, v, w = c[0] * b[1] - c[1] * b[0], a[0] * c[1] - a[1] * c[0], b[0] * a[1] - b[1] * a[0]
            if not ((min(u, v, w) < 0 and max(u, v, w) > 0) or u + v + w == 0):
                out[r] = t
    return out


def shared_edge():
    V, T = _patch()
    return _case(V, T, *_edge_rays())


def coincident_pairs():
    V, T = _patch()
    return _case(V, np.concatenate([T[::-1], T, T[::-1]]), *_edge_rays())


def _closed_rays(V, T, centre, nrandom, seed, outside, outside_step=2):
    """from the centre at EVERY vertex, every edge midpoint (f32) and random directions; from outside: aimed at every
    outside_step-th of those targets, and random with about half missing"""
    V = np.asarray(V, f32)
    E = edges_of(T)
    mid = ((V[E[:, 0]] + V[E[:, 1]]) * f32(0.5)).astype(f32)
    targets = np.concatenate([V, mid])
    O1, D1 = aimed(centre, targets)
    D2 = directions(nrandom, seed)
    O2 = np.broadcast_to(np.asarray(centre, f32), D2.shape)
    O3, D3 = aimed(outside, targets[::outside_step])
    rng = np.random.default_rng(seed + 1)
    c = np.asarray(centre, f64)
    ext = float(np.abs(V.astype(f64) - c).max())
    n4 = max(nrandom // 2, 16)
    O4 = (c + directions(n4, seed + 2).astype(f64) * ext * 4.0).astype(f32)
    D4 = (c + rng.uniform(-1.6, 1.6, (n4, 3)) * ext - O4).astype(f32)   # (targets in a box 1.6 extents wide: about half miss)
    return np.concatenate([O1, O2, O3, O4]), np.concatenate([D1, D2, D3, D4])


def cube_case():
    V, T = cube()
    return _case(V, T, *_closed_rays(V, T, (0.5, 0.5, 0.5), 2048, 11, (2.5, 1.75, -1.25)), colors=position_colors(V))


def sphere_case(n=32, nrandom=2048):
    """The 32^3 marching-cubes sphere: from the centre a ray at every one of its vertices and at the f32 midpoint of every one of
    its edges (no ray slips between triangles), and random ones.  The aimed rays from OUTSIDE are thinned to every 16th target:
    they cost the brute-force model as much as the others and repeat the inside rays' point from one more origin."""
    V, T = mc_sphere(n)
    return _case(V, T, *_closed_rays(V, T, (0.0, 0.0, 0.0), nrandom, 21, (2.5, -1.75, 3.25), outside_step=16))


def small_sphere_all():
    """the same on a 12^3 sphere (a coarser grid), with every second target aimed at from outside too"""
    V, T = mc_sphere(12)
    return _case(V, T, *_closed_rays(V, T, (0.0, 0.0, 0.0), 256, 31, (-2.5, 1.5, 2.0)))


def sphere_inside_random(n=32, nrays=2048):
    """the rays of the pruning condition: random directions from the centre"""
    V, T = mc_sphere(n)
    D = directions(nrays, 41)
    return _case(V, T, np.zeros_like(D), D)


def walk_traps():
    """On the 32^3 sphere's grid (restated: meshsdf_cases.mesh_grid; faces lo + i h in f32): axis-parallel rays lying exactly in
    cell-boundary planes with one and two zero direction components, both directions; exact cell diagonals through cell corners;
    origins on the box faces, its corners and inside; origins 10^6 extents away; rays pointing away; rays that miss the box by
    one ulp and that graze it."""
    V, T = mc_sphere(32)
    g = G.mesh_grid(V, T)
    lo, hi, h, dim = g["lo"], g["hi"], g["h"], g["dim"]
    face = lambda a, i: f32(lo[a] + f32(i) * h)   # noqa: E731
    O, D = [], []
    mids = [dim[a] // 2 for a in range(3)]
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for ib in (1, mids[b], dim[b] - 1):
            for ic in (mids[c], mids[c] + 1):
                for sgn in (1.0, -1.0):
                    # two zero components: along a, in the planes b = face, c = face
                    o = np.zeros(3, f32); o[a] = f32(-3.0 * sgn); o[b] = face(b, ib); o[c] = face(c, ic)
                    d = np.zeros(3, f32); d[a] = sgn
                    O.append(o); D.append(d)
                    # one zero component: in the plane c = face, slanted in (a, b)
                    d2 = np.zeros(3, f32); d2[a] = sgn; d2[b] = f32(0.37 * sgn)
                    O.append(o); D.append(d2)
                    o3 = o.copy(); o3[b] = f32(o3[b] - f32(0.37 * 3.0))   # (this one passes near (face, face) inside the mesh)
                    O.append(o3); D.append(d2)
    # exact cell diagonals through cell corners
    for i0 in ((0, 0, 0), (2, 1, 3), (mids[0], mids[1], 0), (0, mids[1], mids[2])):
        corner = np.array([face(a, i0[a]) for a in range(3)], f32)
        for d in ((1, 1, 1), (-1, -1, -1), (1, -1, 1), (1, 1, 0), (0, -1, 1), (-1, 1, -1)):
            dd = (np.asarray(d, f32) * h).astype(f32)
            O.append((corner - f32(7) * dd).astype(f32)); D.append(dd)
            O.append(corner); D.append(dd)
    # origins on the box faces, its corners, inside
    ctr = ((lo.astype(f64) + hi.astype(f64)) * 0.5).astype(f32)
    for o in ([lo[0], ctr[1], ctr[2]], [hi[0], ctr[1], ctr[2]], [ctr[0], lo[1], ctr[2]], [ctr[0], ctr[1], hi[2]], lo, hi, [lo[0], hi[1], lo[2]],
              [hi[0], lo[1], hi[2]], ctr, [0.3, -0.2, 0.1]):
        o = np.asarray(o, f32)
        for d in directions(6, 51):
            O.append(o); D.append(d)
        O.append(o); D.append((ctr - o).astype(f32) if np.any(ctr != o) else np.array([1, 0, 0], f32))
    # 10^6 extents away, aimed at the mesh
    ext = float((hi.astype(f64) - lo.astype(f64)).max())
    for d in directions(12, 52):
        o = (d.astype(f64) * ext * 1e6).astype(f32)
        for tgt in (ctr, V[17], V[len(V) // 2]):
            O.append(o); D.append((tgt - o).astype(f32))
    # pointing away
    for d in directions(8, 53):
        O.append((d * f32(3.0)).astype(f32)); D.append(d)
    # past the box by one ulp, and grazing it: along x at y = the box's faces and their f32 neighbours
    for y in (hi[1], np.nextafter(hi[1], f32(9)), np.nextafter(hi[1], f32(-9)), lo[1], np.nextafter(lo[1], f32(-9)), np.nextafter(lo[1], f32(9))):
        for z in (ctr[2], hi[2], np.nextafter(hi[2], f32(9))):
            O.append((-3.0, y, z)); D.append((1, 0, 0))
            O.append((3.0, y, z)); D.append((-1, 0.0, 0))
    return _case(V, T, O, D)


def early_exit_trap():
    """Triangle 0 is large: its box spans every cell along the ray, which hits it at x = 9; triangle 1 is small, is hit at x = 5,
    and lies in a later cell.  The answer is triangle 1: a walk that stops at the first cell with a hit answers 0."""
    big = [(0, -10, -0.5), (0, 12, -0.5), (9.9, 0.5, 0.6)]
    small = [(5, 0.3, 0.3), (5, 0.8, 0.3), (5, 0.5, 0.9)]
    Vf, Tf = fillers(250, (0, -10, -0.5), (9.9, 12, 0.6), 0.05, 61, avoid=((0, 0.5, 0.5), (1, 0, 0), 0.6))
    V, T = G.merge(G.soup(np.array([big, small])), (Vf, Tf))
    O = [(-1, 0.5, 0.5), (0.0, 0.5, 0.5), (0.25, 0.5, 0.5), (-1, 0.5, 0.5), (12, 0.5, 0.5)]
    D = [(1, 0, 0), (1, 0, 0), (2, 0, 0), (1, 0.004, -0.003), (-1, 0, 0)]
    return _case(V, T, O, D)


def thin_triangle():
    """a long thin diagonal triangle, binned in every cell of a grid sized by some thousand small triangles, hit once"""
    thin = [(0, 0, 0), (10, 10, 10), (10.02, 10, 10.01)]
    Vf, Tf = fillers(3000, (0, 0, 0), (10.02, 10, 10.01), 0.02, 71, avoid=((0, 0, 0), (1, 1, 1), 0.5))
    V, T = G.merge(G.soup(np.array([thin])), (Vf, Tf))
    p = np.array([5.004, 5.0, 5.002])   # a point of the triangle (between the long edges)
    O, D = aimed((7.0, 7.5, 1.0), [p])      # (the plane's normal is along (1, 1, -2): none of the rays is near it)
    O2, D2 = aimed((3.0, 2.5, 9.5), [p])
    O3, D3 = aimed((5.004, 5.0, 9.0), [p, (5.1, 5.0, 5.0)])
    return _case(V, T, np.concatenate([O, O2, O3]), np.concatenate([D, D2, D3]))


def flat_mesh():
    """the mesh lies in the plane z = 0.25: one grid dimension is 1 and the extent is 0; rays across it and within it"""
    n = 16
    xs = np.linspace(0, 2, n + 1).astype(f32)
    V = np.array([(x, y, 0.25) for y in xs for x in xs], f32)
    T = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            T += [(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)]
    rng = np.random.default_rng(81)
    P = np.concatenate([rng.uniform(-0.3, 2.3, (300, 2)), np.full((300, 1), 0.25)], 1).astype(f32)
    O, D = aimed(np.concatenate([rng.uniform(-1, 3, (300, 2)), rng.choice([-1.5, 0.7, 2.0], (300, 1))], 1), P)
    onv = V[::7]
    O2, D2 = aimed((1.0, 1.0, 3.0), onv)
    within_o = [(-1, 0.5, 0.25), (0.5, 0.5, 0.25), (-1, -1, 0.25), (3, 1.0, 0.25), (1.0, 1.0, 0.25)]
    within_d = [(1, 0, 0), (1, 0.25, 0), (1, 1, 0), (-1, 0, 0), (0, 0, 1)]
    return _case(V, np.array(T, i32), np.concatenate([O, O2, np.array(within_o, f32)]), np.concatenate([D, D2, np.array(within_d, f32)]))


def ranges():
    """a known hit at t = 0.5 (the unit cube from its centre along +x; the wall behind is at t = -0.5); every range is its own call"""
    V, T = cube()
    O, D = [(0.5, 0.5, 0.5), (0.5, 0.25, 0.625), (0.5, 0.5, 0.5)], [(1, 0, 0), (1, 0, 0), (-2, 0, 0)]
    t = f32(0.5)
    below, above = np.nextafter(t, f32(0)), np.nextafter(t, f32(1))
    out = {}
    for name, (a, b) in {"tmax_below": (0, below), "tmax_at": (0, t), "tmax_above": (0, above), "tmin_below": (below, 10), "tmin_at": (t, 10),
                         "tmin_above": (above, 10), "point": (t, t), "to_inf": (0, INF), "behind": (-10, 0), "behind_far": (-INF, -0.4),
                         "all": (-INF, INF)}.items():
        out["range_" + name] = (lambda a=a, b=b: _case(V, T, O, D, a, b))
    return out


def _scaled(factor):
    c = cube_case()
    D = (c["D"][:600] * f32(factor)).astype(f32)
    return _case(c["V"], c["T"], c["O"][:600], D, 0.0, INF)


def far_mesh():
    """a unit cube at coordinates around 10^6 (the f32 spacing there is 1/16)"""
    V, T = cube()
    V = (V + f32(1e6)).astype(f32)
    D = directions(400, 91)
    Oc = np.broadcast_to(np.array([1e6 + 0.5] * 3, f32), D.shape)
    O2, D2 = aimed((1e6 + 4.0, 1e6 - 2.0, 1e6 + 0.25), V)
    return _case(V, T, np.concatenate([Oc, O2]), np.concatenate([D, D2]))


def bad_rays():
    """a NaN or an infinite component in each position, a zero direction; good rays between them"""
    V, T = cube()
    good_d = directions(64, 95)
    O, D = [], []
    k = 0
    for bad in (np.nan, np.inf, -np.inf):
        for pos in range(6):
            o, d = np.array([0.5, 0.5, 0.5], f32), good_d[k % 64].copy()
            (o if pos < 3 else d)[pos % 3] = bad
            O.append(o); D.append(d)
            O.append((0.5, 0.5, 0.5)); D.append(good_d[(k + 7) % 64])
            k += 1
    O.append((0.5, 0.5, 0.5)); D.append((0, 0, 0))
    O.append((0.5, 0.5, 0.5)); D.append((-0.0, 0.0, -0.0))
    for j in range(40):
        O.append((0.5, 0.5, 0.5)); D.append(good_d[j])
    return _case(V, T, O, D)


def _count(n):
    c = cube_case()
    return _case(c["V"], c["T"], c["O"][100:100 + n], c["D"][100:100 + n])


CASES = {
    "single_triangle": single_triangle,
    "shared_edge": shared_edge,
    "coincident_pairs": coincident_pairs,
    "cube": cube_case,
    "small_sphere_all": small_sphere_all,
    "sphere": sphere_case,
    "sphere_inside_random": sphere_inside_random,
    "walk_traps": walk_traps,
    "early_exit_trap": early_exit_trap,
    "thin_triangle": thin_triangle,
    "flat_mesh": flat_mesh,
    "scale_1e-30": lambda: _scaled(1e-30),
    "scale_1e30": lambda: _scaled(1e30),
    "far_mesh": far_mesh,
    "bad_rays": bad_rays,
}
CASES.update(ranges())
CASES.update({f"count_{n}": (lambda n=n: _count(n)) for n in (0, 1, 255, 256, 257)})

CLOSED = ("cube", "small_sphere_all", "sphere")          # every ray from the centre hits; crossings from outside are even
OUTSIDE_RANDOM = {"cube": 1024, "small_sphere_all": 128, "sphere": 1024}   # the last rays of a closed case: random, from outside
EVERY_RAY_HITS = ("shared_edge", "coincident_pairs")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def model(name, flags=0):
    """the numpy model's answer, computed once per process and shared"""
    from tests import mesh_ray_model as M
    c = case(name)
    return M.cast(c["V"], c["T"], c["O"], c["D"], c["tmin"], c["tmax"], flags)


# ---- render cases: (mesh, colours, width, height, camera (position, target, up), near, far) ---------------------------------------
def _render(mesh, colors, w, h, cam, near=1.0, far=100.0):
    V, T = mesh()
    return {"V": V, "T": T, "colors": position_colors(V) if colors else None, "width": w, "height": h, "camera": cam, "near": near, "far": far}


def _cube_centred():
    V, T = cube(-1.0, 1.0)
    return V, T


_SPH = lambda: mc_sphere(32)   # noqa: E731
_CAM = ((1.5, 0.9, 2.4), (0, 0, 0), (0, 1, 0))
RENDER = {}
for _w, _h in ((1, 1), (2, 2), (1, 7), (257, 3), (64, 48)):
    RENDER[f"cube_{_w}x{_h}"] = (lambda w=_w, h=_h: _render(_cube_centred, False, w, h, _CAM))
    RENDER[f"sphere_colors_{_w}x{_h}"] = (lambda w=_w, h=_h: _render(_SPH, True, w, h, _CAM))
RENDER["cube_colors_64x48"] = lambda: _render(_cube_centred, True, 64, 48, _CAM)
RENDER["sphere_64x48"] = lambda: _render(_SPH, False, 64, 48, _CAM)
RENDER["inside_sphere"] = lambda: _render(_SPH, True, 33, 21, ((0.1, 0.2, 0.3), (1, 0.5, -0.25), (0, 1, 0)), 0.125, 100.0)
RENDER["far_all_sky"] = lambda: _render(_SPH, False, 32, 24, ((0, 0, 50), (0, 0, 0), (0, 1, 0)), 1.0, 40.0)
RENDER["near_past_front"] = lambda: _render(_cube_centred, True, 40, 30, ((0, 0, 5), (0, 0, 0), (0, 1, 0)), 4.5, 100.0)


@functools.lru_cache(maxsize=None)
def render_case(name):
    from sdfkit_amd.raymarch import Matrix4x4, RayMarcher
    c = RENDER[name]()
    rm = RayMarcher(c["width"], c["height"], None)
    rm.ViewTransform = Matrix4x4.CreateLookAt(*c["camera"])
    rm.NearPlaneDistance, rm.FarPlaneDistance = c["near"], c["far"]
    c["cam"], c["vpi"] = rm.camera()
    return c


@functools.lru_cache(maxsize=None)
def render_model(name):
    from tests import mesh_ray_model as M
    c = render_case(name)
    return M.render(c["V"], c["T"], c["colors"], c["width"], c["height"], c["cam"], c["vpi"], c["near"], c["far"])


# ---- the host program (tests/cpp/mesh_ray_host.cpp): the header's walk on the CPU ---------------------------------------------------
def build_host(directory, sanitize=False):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(directory), "mesh_ray_host" + ("_san" if sanitize else ""))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall"] + extra + [os.path.join(root, "tests", "cpp", "mesh_ray_host.cpp"), "-o", exe])
    return exe


def _run_host(exe, mode, blob, directory, tag):
    import os
    import subprocess
    src, dst = os.path.join(str(directory), f"{tag}.in"), os.path.join(str(directory), f"{tag}.out")
    with open(src, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "mesh ray ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    out = np.fromfile(dst, np.int64)
    head = {"tests": int(out[1]), "differs": int(out[2]), "dim": tuple(int(x) for x in out[3:6]), "entries": int(out[6]), "n": int(out[7])}
    return head, out[8:].reshape(-1, 6)


def _bits_f32(col):
    return col.astype(np.uint32).view(f32)


def host_cast(exe, directory, c, flags=0, tag="cast"):
    """-> (head, triangle, distance, weights, tests per ray) of the host walk"""
    import struct
    blob = struct.pack("<4q2f", len(c["V"]), len(c["T"]), len(c["O"]), flags, c["tmin"], c["tmax"]) + c["V"].tobytes() + c["T"].tobytes() + \
        c["O"].tobytes() + c["D"].tobytes()
    head, rows = _run_host(exe, "cast", blob, directory, tag)
    return head, rows[:, 0].astype(i32), _bits_f32(rows[:, 1]), np.stack([_bits_f32(rows[:, k]) for k in (2, 3, 4)], -1).reshape(-1, 3), rows[:, 5]


def host_render(exe, directory, c, tag="render"):
    """-> (head, depth, rgb, triangle) images of the host walk"""
    import struct
    cols = c["colors"]
    blob = struct.pack("<5q2f", len(c["V"]), len(c["T"]), c["width"], c["height"], int(cols is not None), c["near"], c["far"]) + \
        np.asarray(c["cam"], f32).tobytes() + np.asarray(c["vpi"], f32).tobytes() + c["V"].tobytes() + c["T"].tobytes() + \
        (b"" if cols is None else cols.tobytes())
    head, rows = _run_host(exe, "render", blob, directory, tag)
    h, w = c["height"], c["width"]
    return head, _bits_f32(rows[:, 1]).reshape(h, w), np.stack([_bits_f32(rows[:, k]) for k in (2, 3, 4)], -1).reshape(h, w, 3), \
        rows[:, 0].astype(i32).reshape(h, w)
