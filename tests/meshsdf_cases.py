"""Adversarial meshes and queries for the triangle-mesh closest search and sign (tests/test_gpu_meshsdf_search.py): deterministic
generators with fixed seeds -- float32 vertices, int32 indices -- and a restatement of the search grid (csrc/points_grid.h
grid_for_box / cell_of) in numpy, so that a case can say on the CPU which cells its triangles and queries fall into."""
import numpy as np

from tests import meshsdf_model as M

f32 = np.float32
f64 = np.float64


# ---- the search grid, restated ------------------------------------------------------------------------------------------
K_MAX_CELLS = 1 << 25
K_MAX_AXIS = 1 << 24


def grid_for_box(lo, hi, n):
    """points_grid.h grid_for_box: the smallest cell edge whose cell count stays within min(n, 2^25).  All binary64, as there."""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    ext = hi.astype(f64) - lo.astype(f64)
    emax = float(ext.max())
    amax = float(max(np.abs(lo.astype(f64)).max(), np.abs(hi.astype(f64)).max()))
    target = float(min(max(int(n), 1), K_MAX_CELLS))

    def cells_at(h):
        c = 1.0
        for a in range(3):
            ca = np.floor(ext[a] / h) + 1.0
            if ca > K_MAX_AXIS:
                return np.inf
            c *= ca
        return c

    if emax <= 0:
        h = 1.0
    else:
        hi_h, lo_h = emax * 1.000001, emax / (2.0 * np.cbrt(target) + 2.0)
        while cells_at(lo_h) <= target:
            lo_h *= 0.5
        for _ in range(60):
            mid = 0.5 * (lo_h + hi_h)
            if cells_at(mid) <= target:
                hi_h = mid
            else:
                lo_h = mid
        h = hi_h
    hf = f32(h)
    dim = [int(min(max(np.floor(ext[a] / f64(hf)) + 1.0, 1.0), K_MAX_AXIS)) for a in range(3)]
    while dim[0] * dim[1] * dim[2] > K_MAX_CELLS:
        dim = [max(1, d - 1) for d in dim]
    return {"lo": lo, "hi": hi, "h": hf, "inv_h": f32(1.0 / f64(hf)), "dim": tuple(dim),
            "slack": f32((emax + amax) * 2.0 ** -19 + f64(hf) * 2.0 ** -20)}


def mesh_grid(V, T):
    """The grid lib_trimesh.hip builds for (V, T): the box of the triangles' vertices, sized from the triangle count."""
    V = np.asarray(V, f32).reshape(-1, 3)
    P = V[np.asarray(T, np.int64).reshape(-1)]
    return grid_for_box(P.min(0), P.max(0), len(P) // 3)


def cell_of(G, X):
    """points_grid.h cell_of per axis, f32 as there: (n, 3) coordinates -> (n, 3) cells.  fmaxf / fminf return the other operand
    of a NaN (np.fmax / np.fmin; np.maximum would hand the NaN on), so a NaN -- a NaN coordinate, or 0 * inf where inv_h has
    overflowed -- lands in cell 0; the truncation comes after the clamp."""
    X = np.asarray(X, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        t = (X - G["lo"][None]) * G["inv_h"]
    t = np.fmin(np.fmax(t, f32(0)), f32(K_MAX_AXIS))
    return np.minimum(t.astype(np.int64), np.asarray(G["dim"], np.int64)[None] - 1)


def entries(G, V, T):
    """The number of (triangle, cell) pairs of the binning: every cell a triangle's AABB overlaps."""
    P = np.asarray(V, f32).reshape(-1, 3)[np.asarray(T, np.int64).reshape(-1, 3)]
    c0, c1 = cell_of(G, P.min(1)), cell_of(G, P.max(1))
    return int(np.prod(c1 - c0 + 1, axis=1).sum())


# ---- helpers ------------------------------------------------------------------------------------------------------------
def soup(tris):
    """(n, 3, 3) triangle corners -> (V, T) with three vertices of its own per triangle."""
    tris = np.asarray(tris, f32)
    return np.ascontiguousarray(tris.reshape(-1, 3)), np.arange(3 * len(tris), dtype=np.int32)


def merge(*meshes):
    Vs, Ts, off = [], [], 0
    for V, T in meshes:
        V = np.asarray(V, f32).reshape(-1, 3)
        Vs.append(V)
        Ts.append(np.asarray(T, np.int32).reshape(-1) + off)
        off += len(V)
    return np.ascontiguousarray(np.concatenate(Vs)), np.ascontiguousarray(np.concatenate(Ts).astype(np.int32))


def _small_triangles(rng, centres, e0, e1):
    """One triangle about every centre, edges of about e0 .. e1, any orientation."""
    n = len(centres)
    u = rng.normal(size=(n, 3, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    r = rng.uniform(e0, e1, (n, 1, 1)) / np.sqrt(3.0)   # (corners on a sphere of radius e / sqrt 3: edges of about e)
    return centres[:, None, :] + u * r


def translated(V, offset):
    """The mesh moved by `offset`, rounded to f32: what the library and the model both see."""
    return np.ascontiguousarray((np.asarray(V, f32) + np.asarray(offset, f32)[None]).astype(f32))


# ---- 1. mixed sizes -----------------------------------------------------------------------------------------------------
BIG = np.array([[[-1.5, -1.0, -0.8], [1.5, -0.6, 0.1], [0.2, 1.5, 0.9]],
                [[-1.2, 1.4, -1.0], [1.3, 1.0, 0.6], [-0.3, -1.5, 0.4]],
                [[-1.4, -0.2, 1.2], [1.4, 0.5, -1.1], [0.0, -1.4, -0.3]],
                [[0.1, -1.3, 1.3], [-0.2, 1.5, 0.2], [1.1, 0.2, -1.4]]], f64)


def mixed_sizes(n_small=1500, seed=101):
    """n_small triangles with edges of 0.01 .. 0.03 scattered in [-1, 1]^3 and four with edges of about 3 that cut through the
    whole box: two of the large ones at the lowest indices, two at the highest."""
    rng = np.random.default_rng(seed)
    small = _small_triangles(rng, rng.uniform(-0.97, 0.97, (n_small, 3)), 0.01, 0.03)
    big = BIG + rng.uniform(-0.02, 0.02, BIG.shape)
    return soup(np.concatenate([big[:2], small, big[2:]]))


def boundary_traps(V, T, want=12, seed=108):
    """Replaces 2 * want of the small triangles of a mixed-size soup (its box, count and so its grid unchanged) by pairs that only
    the slack of the shell bound keeps apart.  A trap sits at a cell boundary c along one axis whose f32 position in the shell
    bound, bf = lo + f32(c) * h, lies a few f32 steps ABOVE coordinates that cell_of still puts into cell c: a small triangle T1,
    perpendicular to the axis, at such a coordinate x1 < bf (binned in cell c only); the query at bf - g in cell c - 1; a second
    triangle T2 in cell c - 1 on the query's other side at a distance D with g - (bf - x1) < D < g (1 - 2^-19).  T1 is the closest
    triangle, and T2 is within the bound that a search without slack computes for cell c (g^2 (1 - 2^-18)): such a search stops
    at T2.  Returns (V, T, queries, winners)."""
    rng = np.random.default_rng(seed)
    V = np.array(V, f32).reshape(-1, 3).copy()
    T = np.asarray(T, np.int32).reshape(-1)
    G = mesh_grid(V, T)
    nt = len(T) // 3
    queries, winners, slot = [], [], 2      # (triangles 0, 1 and the last two are the large ones)
    g = 0.002
    for a in (2, 1, 0):
        for c in range(1, G["dim"][a]):
            if len(queries) >= want:
                break
            bf = f32(G["lo"][a] + f32(f32(c) * G["h"]))
            x1, k = bf, 0
            while True:      # the lowest coordinate below bf that cell_of still puts into cell c
                nx = np.nextafter(x1, f32(-np.inf))
                p = G["lo"].copy()
                p[a] = nx
                if cell_of(G, p[None])[0, a] != c:
                    break
                x1, k = nx, k + 1
            if k < 2:
                continue
            qa = f32(f64(bf) - g)
            d1 = f64(x1) - f64(qa)                                   # the distance of T1
            bound = f64(f32(bf - qa)) * (1.0 - 2.0 ** -19)           # below it, T2 is within the slack-free bound of cell c
            x2 = f32(f64(qa) - 0.5 * (d1 + bound))
            D = f64(qa) - f64(x2)
            if not (d1 < D < bound):
                continue
            centre = G["lo"].astype(f64) + (rng.integers(2, np.array(G["dim"]) - 2) + 0.5) * f64(G["h"])   # mid-cell on the other axes
            o = [b for b in range(3) if b != a]

            def plate(x, r=0.01):      # a small triangle in the plane (axis a) = x about the centre
                P = np.empty((3, 3))
                P[:, a], P[:, o[0]], P[:, o[1]] = x, centre[o[0]] + np.array([-r, r, 0.0]), centre[o[1]] + np.array([-r, -r, r])
                return P.astype(f32)

            q = centre.copy()
            q[a] = qa
            V[3 * slot:3 * slot + 3] = plate(x1)
            V[3 * (nt - 3 - slot):3 * (nt - 3 - slot) + 3] = plate(x2)
            queries.append(q.astype(f32))
            winners.append(slot)
            slot += 1
    return np.ascontiguousarray(V), T, np.array(queries, f32), np.array(winners, np.int32)


def stops_early_without_slack(G, V, T, q):
    """On the CPU: would the shell walk, with the slack taken out of its shell bound, stop after the query's own cell?  The best
    d2 among the triangles binned into that cell against the bound of shell 0 as lib_trimesh.hip computes it in f32 (the query
    inside the box), slack = 0.  Returns (stops, that best triangle)."""
    Vd = np.asarray(V, f32).reshape(-1, 3)
    P = Vd[np.asarray(T, np.int64).reshape(-1, 3)]
    c0, c1 = cell_of(G, P.min(1)), cell_of(G, P.max(1))
    q = np.asarray(q, f32)
    c = cell_of(G, q[None])[0]
    own = np.nonzero(np.all((c0 <= c) & (c <= c1), axis=1))[0]
    if not len(own):
        return False, -1
    d2, _, _ = M.closest_on_triangle(q.astype(f64)[None], *[P[own, k].astype(f64) for k in range(3)])
    lb = np.inf
    for a in range(3):
        g0 = max(f32(q[a] - f32(G["lo"][a] + f32(f32(c[a]) * G["h"]))), f32(0)) if c[a] - 1 >= 0 else f32(np.inf)
        g1 = max(f32(f32(G["lo"][a] + f32(f32(c[a] + 1) * G["h"])) - q[a]), f32(0)) if c[a] + 1 < G["dim"][a] else f32(np.inf)
        gm = min(g0, g1)
        lb = min(lb, f64(f32(gm * gm)))
    return bool(lb * (1.0 - 2.0 ** -18) > d2.min()), int(own[np.argmin(d2)])


# ---- 2. flat and needle boxes -------------------------------------------------------------------------------------------
def sheet(n=30, seed=102, scale=(1.0, 1.0)):
    """A jittered n x n sheet of vertices, every one at z = 0.25 exactly: 2 (n - 1)^2 triangles in a box of no z extent.
    scale: the xy extent."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    xy = np.stack([i, j], -1).astype(f64) + rng.uniform(-0.3, 0.3, (n, n, 2))
    xy = (xy - xy.reshape(-1, 2).min(0)) / (xy.reshape(-1, 2).max(0) - xy.reshape(-1, 2).min(0))
    V = np.concatenate([xy.reshape(-1, 2) * np.asarray(scale), np.full((n * n, 1), 0.25)], 1).astype(f32)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    T = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)]).astype(np.int32)
    return np.ascontiguousarray(V), np.ascontiguousarray(T.reshape(-1))


def tube(length=100.0, radius=0.5, along=100, around=8, seed=103):
    """An open tube along x: extent of about length x 2 radius x 2 radius, 2 * along * around triangles."""
    rng = np.random.default_rng(seed)
    k, s = np.meshgrid(np.arange(along + 1), np.arange(around), indexing="ij")
    ang = 2 * np.pi * (s + 0.5 * (k % 2)) / around
    x = length * k / along + rng.uniform(-0.2, 0.2, k.shape) * (length / along) * ((k > 0) & (k < along))
    V = np.stack([x, radius * np.cos(ang), radius * np.sin(ang)], -1).reshape(-1, 3).astype(f32)
    a = (k[:-1] * around + s[:-1]).reshape(-1)
    b = (k[:-1] * around + (s[:-1] + 1) % around).reshape(-1)
    T = np.concatenate([np.stack([a, a + around, b], 1), np.stack([b, a + around, b + around], 1)]).astype(np.int32)
    return np.ascontiguousarray(V), np.ascontiguousarray(T.reshape(-1))


# ---- 4. two clusters and a void -----------------------------------------------------------------------------------------
def two_clusters(n_each=700, gap=40.0, seed=104):
    """Two blobs of n_each small triangles, each of diameter 1, their centres `gap` diameters apart along x."""
    rng = np.random.default_rng(seed)
    blobs = []
    for cx in (0.0, gap):
        d = rng.normal(size=(n_each, 3))
        d *= (0.5 * rng.uniform(0, 1, (n_each, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        blobs.append(_small_triangles(rng, d + [cx, 0.0, 0.0], 0.02, 0.06))
    return soup(np.concatenate(blobs))


def cluster_queries(gap=40.0, seed=105):
    """In the void between the blobs, beside each of them, and on the far side of each."""
    rng = np.random.default_rng(seed)
    void = np.stack([rng.uniform(1.0, gap - 1.0, 120), rng.uniform(-1.5, 1.5, 120), rng.uniform(-1.5, 1.5, 120)], 1)
    mid = np.array([[gap / 2, 0, 0], [gap / 2, 0.25, -0.125], [gap / 2 - 0.5, 0, 0], [gap / 2 + 0.5, 0, 0]])
    beside = np.concatenate([np.stack([rng.uniform(-0.7, 0.7, 40) + cx, rng.uniform(-3, 3, 40), rng.uniform(-3, 3, 40)], 1) for cx in (0.0, gap)])
    far = np.concatenate([np.stack([cx + sg * rng.uniform(0.6, 30, 30), rng.uniform(-2, 2, 30), rng.uniform(-2, 2, 30)], 1)
                          for cx, sg in ((0.0, -1.0), (gap, 1.0))])
    return np.concatenate([void, mid, beside, far]).astype(f32)


# ---- 5. exact ties across shells ----------------------------------------------------------------------------------------
LATTICE = (10, 9, 8)
SPACING, SIZE = 1.0 / 8, 1.0 / 32


def tie_lattice(variant="shuffled", seed=106):
    """Identical small triangles on a lattice of dyadic coordinates (spacing 1/8, size 1/32), flat in z and symmetric in x, in
    an order shuffled with a fixed seed.  variant: "shuffled"; "appended" / "prepended": every triangle twice, the copies (with
    vertices of their own, in another shuffled order) after / before the originals."""
    rng = np.random.default_rng(seed)
    i, j, k = [a.reshape(-1) for a in np.meshgrid(*[np.arange(n) for n in LATTICE], indexing="ij")]
    p = np.stack([i, j, k], 1) * SPACING
    s = SIZE / 2
    corners = np.array([[-s, -s, 0.0], [s, -s, 0.0], [0.0, s, 0.0]])
    tris = p[:, None, :] + corners[None]
    first, second = tris[rng.permutation(len(tris))], tris[rng.permutation(len(tris))]
    if variant == "shuffled":
        return soup(first)
    return soup(np.concatenate([first, second] if variant == "appended" else [second, first]))


def tie_queries(seed=107):
    """Dyadic points with several triangles at exactly the same distance: midway between two lattice planes in z (a tie of the
    triangle below and the one above), also midway in x or y, the cell centres of the lattice, and the lattice points."""
    rng = np.random.default_rng(seed)
    n = 260
    base = np.stack([rng.integers(0, LATTICE[a] - 1, n) for a in range(3)], 1) * SPACING
    fine = rng.integers(-8, 9, (n, 3)) / 128.0                      # dyadic offsets up to half a spacing
    q = base + fine
    kind = rng.integers(0, 5, n)
    half = SPACING / 2
    q[:, 2] = np.where(kind <= 3, base[:, 2] + half, q[:, 2])        # midway in z
    q[:, 0] = np.where((kind == 1) | (kind == 3), base[:, 0] + half, q[:, 0])   # and in x
    q[:, 1] = np.where((kind == 2) | (kind == 3), base[:, 1] + half, q[:, 1])   # and in y
    q[kind == 4] = base[kind == 4]                                      # lattice points
    return q.astype(f32)


def tie_statistics(V, T, Q, G):
    """On the model: for every query, the triangles at the minimal d2.  Returns (tied, other_row, later_shell): the number of
    queries with two or more of them; of those, the number whose winner (the lowest index) has its closest point in another cell
    row (y, z) than the runner-up's (the next index); and the number whose winner is first met in a later Chebyshev shell of
    cells around the query than some other triangle at that distance."""
    Vd = np.asarray(V, f32).reshape(-1, 3).astype(f64)
    Tt = np.asarray(T, np.int64).reshape(-1, 3)
    A, B, Cc = Vd[Tt[:, 0]], Vd[Tt[:, 1]], Vd[Tt[:, 2]]
    lo, hi = np.minimum(np.minimum(A, B), Cc).astype(f32), np.maximum(np.maximum(A, B), Cc).astype(f32)
    c0, c1 = cell_of(G, lo), cell_of(G, hi)
    qc = cell_of(G, Q)
    tied = other_row = later_shell = 0
    for q, c in zip(np.asarray(Q, f32).astype(f64), qc):
        d2, cp, _ = M.closest_on_triangle(q[None], A, B, Cc)
        w = np.nonzero(d2 == d2.min())[0]
        if len(w) < 2:
            continue
        tied += 1
        rows = cell_of(G, cp[w[:2]].astype(f32))[:, 1:]
        other_row += int(np.any(rows[0] != rows[1]))
        shell = np.max(np.maximum(np.maximum(c0[w] - c, c - c1[w]), 0), axis=1)   # the first shell that meets the triangle
        later_shell += int(shell[0] > shell[1:].min())
    return tied, other_row, later_shell


# ---- 6. nested shells ---------------------------------------------------------------------------------------------------
def nested_boxes(halves):
    """Concentric closed boxes about the origin; halves: (k, 3) half sizes."""
    return merge(*[M.box_mesh(-np.asarray(h, f32), np.asarray(h, f32)) for h in halves])


def nested_boxes_between(los, his):
    """Closed boxes [los[k], his[k]] (any nesting the caller chose)."""
    return merge(*[M.box_mesh(l, h) for l, h in zip(los, his)])


# ---- queries ------------------------------------------------------------------------------------------------------------
def box_of(V, T):
    P = np.asarray(V, f32).reshape(-1, 3)[np.asarray(T, np.int64).reshape(-1)]
    return P.min(0).astype(f64), P.max(0).astype(f64)


def random_queries(V, T, n, seed):
    """Uniform in the mesh's box enlarged by 50 % (about its centre; by the largest extent along an axis of no extent)."""
    lo, hi = box_of(V, T)
    c, e = 0.5 * (lo + hi), hi - lo
    e = np.where(e > 0, e, e.max())
    rng = np.random.default_rng(seed)
    return (c + rng.uniform(-0.75, 0.75, (n, 3)) * e).astype(f32)


def surface_queries(V, T, n, seed):
    """n mesh vertices and n edge midpoints (rounded to f32)."""
    rng = np.random.default_rng(seed)
    V = np.asarray(V, f32).reshape(-1, 3)
    Tt = np.asarray(T, np.int64).reshape(-1, 3)
    t = Tt[rng.integers(0, len(Tt), n)]
    e = rng.integers(0, 3, n)
    a, b = V[t[np.arange(n), e]].astype(f64), V[t[np.arange(n), (e + 1) % 3]].astype(f64)
    return np.concatenate([V[Tt.reshape(-1)[rng.integers(0, Tt.size, n)]], (0.5 * (a + b)).astype(f32)]).astype(f32)


def outside_queries(V, T):
    """Along every axis and the eight corner directions at 10, 1000 and 10^6 times the extent from the box's centre, and the points
    exactly on the corners and the face centres of the mesh's bounding box."""
    lo, hi = box_of(V, T)
    c, ext = 0.5 * (lo + hi), float((hi - lo).max())
    dirs = [s * np.eye(3)[a] for a in range(3) for s in (-1.0, 1.0)]
    dirs += [np.array([sx, sy, sz], f64) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    q = [c + d * (k * ext) for k in (10.0, 1000.0, 1e6) for d in dirs]
    q += [np.where([i & 1, i & 2, i & 4], hi, lo) for i in range(8)]
    for a in range(3):
        for side in (lo, hi):
            p = c.copy()
            p[a] = side[a]
            q.append(p)
    return np.array(q).astype(f32)
