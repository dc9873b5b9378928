"""Adversarial point clouds and queries for the KdTree's shell walk (csrc/points_walk.h), and a numpy restatement of that walk
(tests/test_points_walk_model.py on the CPU, tests/test_gpu_points_walk.py on the MI355X): deterministic generators with fixed
seeds, float32 out.  Not a test module.

The walk's answers must equal brute force whatever the cloud; what makes them so is its lower bound (lb_sq over the f32 cell
boundaries lo + (float)c * h, minus the absolute slack of points_grid.h and |q| * 2^-20) and its stopping rule (points_knn.h
walk_done).  The cases put points within rounding distance of a cell boundary (traps), move the cloud far from the origin, scale it
until d2 is denormal, zero or infinite, and stretch the grid into a needle, a sheet and two clusters with a void between.
walk() restates the device's walk operation by operation, so that a test can say how many candidates the device has to visit --
no fewer (a bound that is not conservative) and no more (a bound that is too slack) -- and what a walk without slack would answer.
"""
import numpy as np

from tests import meshsdf_cases as MC
from tests.meshsdf_cases import cell_of, grid_for_box   # (the grid is restated there, once)

f32, f64 = np.float32, np.float64
u32, u64 = np.uint32, np.uint64
FLT_MAX = np.finfo(f32).max
KEY_INF = u64(0x7f800000) << u64(32)       # points_knn.h kKeyInf: (d2 = +inf, index 0)
N_POINTS = 4000


# ---- the grid of a cloud ------------------------------------------------------------------------------------------------
def cloud_grid(P):
    """The grid lib_points.hip builds for the static points P: their box, sized from their count."""
    P = np.asarray(P, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return grid_for_box(P.min(0), P.max(0), len(P))


def boundary(G, a, c):
    """The f32 position of the boundary below cell c along axis a, as the walk computes it: lo + (float)c * h."""
    with np.errstate(all="ignore"):
        return f32(G["lo"][a] + f32(f32(c) * G["h"]))


# ---- the key arithmetic of points_knn.h -----------------------------------------------------------------------------------
def dist2(q, P):
    """d2 = (dx*dx + dy*dy) + dz*dz in f32, no FMA: q (3,), P (n, 3) -> (n,)."""
    with np.errstate(all="ignore"):
        d = q[None, :] - P
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def pack_keys(d2, index):
    return np.ascontiguousarray(d2, f32).view(u32).astype(u64) << u64(32) | np.asarray(index).astype(u32).astype(u64)


def key_d2(keys):
    return (np.asarray(keys, u64) >> u64(32)).astype(u32).view(f32)


def key_index(keys):
    return (np.asarray(keys, u64) & u64(0xffffffff)).astype(u32).view(np.int32)


def sqrt_rn(d2):
    return np.sqrt(np.asarray(d2, f32).astype(f64)).astype(f32)


def radius_d2_bound(r):
    """points_knn.h radius_d2_bound: the largest finite d2 whose correctly rounded root does not exceed r (r >= 0 or +inf)."""
    r = f32(r)
    with np.errstate(all="ignore"):
        rr = f64(r) * f64(r)
        t = FLT_MAX if rr >= f64(FLT_MAX) else f32(rr)
        while t > 0 and sqrt_rn(t) > r:
            t = np.nextafter(t, f32(0))
        while t < FLT_MAX and sqrt_rn(np.nextafter(t, f32(np.inf))) <= r:
            t = np.nextafter(t, f32(np.inf))
    return f32(t)


# ---- the walk, restated ---------------------------------------------------------------------------------------------------
class Walk:
    """points_walk.h shell_walk with points_knn.h's KnnVisitor over the static points P: the grid, and every point's cell."""

    def __init__(self, P):
        self.P = np.ascontiguousarray(np.asarray(P, f32).reshape(-1, 3))
        self.G = cloud_grid(self.P)
        self.cells = cell_of(self.G, self.P)
        self.index = np.arange(len(self.P))

    def lower_bounds(self, q, c, rmax, slack=True):
        """lb_sq after shell r for r = 0 .. rmax, every f32 operation rounded as the header writes it -> (rmax + 1,) f32."""
        G = self.G
        inf = f32(np.inf)
        with np.errstate(all="ignore"):
            sl = f32(G["slack"] + f32(np.abs(q).max() * f32(2.0 ** -20))) if slack else f32(0)
            r = np.arange(rmax + 1)
            base2, gm = [], []
            for a in range(3):
                out = np.fmax(np.fmax(G["lo"][a] - q[a], q[a] - G["hi"][a]) - sl, f32(0))
                base2.append(f32(out * out))
                below = np.fmax((q[a] - (G["lo"][a] + (c[a] - r).astype(f32) * G["h"])) - sl, f32(0))
                above = np.fmax(((G["lo"][a] + (c[a] + r + 1).astype(f32) * G["h"]) - q[a]) - sl, f32(0))
                g0 = np.where(c[a] - r - 1 >= 0, below, inf).astype(f32)
                g1 = np.where(c[a] + r + 1 < G["dim"][a], above, inf).astype(f32)
                gm.append(np.fmin(g0, g1))
            best = np.full(rmax + 1, inf, f32)
            for a in range(3):
                rest = f32(base2[(a + 1) % 3] + base2[(a + 2) % 3])
                best = np.fmin(best, gm[a] * gm[a] + rest)
        return best

    def candidates_by_ranges(self, q, last):
        """The candidates of shells 0 .. last counted as the header enumerates them: per (z, y) row of the shell either the one
        contiguous range of cells x0 .. x1 (a full row) or the row's two end cells, through the table of cell starts."""
        q = np.asarray(q, f32).reshape(3)
        gx, gy, gz = self.G["dim"]
        key = (self.cells[:, 2] * gy + self.cells[:, 1]) * gx + self.cells[:, 0]
        starts = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=gx * gy * gz))])
        c = cell_of(self.G, q[None])[0]
        ncand = 0
        for r in range(last + 1):
            z0, z1 = max(c[2] - r, 0), min(c[2] + r, gz - 1)
            y0, y1 = max(c[1] - r, 0), min(c[1] + r, gy - 1)
            x0, x1 = max(c[0] - r, 0), min(c[0] + r, gx - 1)
            for z in range(z0, z1 + 1):
                zf = z == c[2] - r or z == c[2] + r
                for y in range(y0, y1 + 1):
                    full = zf or y == c[1] - r or y == c[1] + r
                    row = (z * gy + y) * gx
                    for part in range(1 if full else 2):
                        if full:
                            xa, xb = x0, x1
                        else:
                            xa = xb = c[0] - r if part == 0 else c[0] + r
                            if xa < 0 or xa >= gx:
                                continue
                        ncand += int(starts[row + xb + 1] - starts[row + xa])
        return ncand

    def query(self, q, k, d2_bound=FLT_MAX, slack=True):
        """The walk of one query for the k least keys within d2_bound (k None: every key within it, the radius kernels' visitor)
        -> (keys ascending (uint64; at most k), candidates, last shell).  A non-finite query is not walked: ((), 0, -1)."""
        q = np.asarray(q, f32).reshape(3)
        if not np.isfinite(q).all():
            return np.zeros(0, u64), 0, -1
        G = self.G
        dim = np.asarray(G["dim"], np.int64)
        c = cell_of(G, q[None])[0]
        rmax = int(np.maximum(c, dim - 1 - c).max())
        # the cells of shell r are those at Chebyshev distance r from c (the walk clamps its ranges to the grid, and every point
        # lies in the cell the build gave it): the candidates of shell r are the points whose cell is at that distance
        shell = np.abs(self.cells - c[None]).max(axis=1)
        order = np.argsort(shell, kind="stable")
        upto = np.cumsum(np.bincount(shell, minlength=rmax + 1))
        keys = pack_keys(dist2(q, self.P), self.index)[order]
        lb = self.lower_bounds(q, c, rmax, slack)
        bound_key = pack_keys(f32(d2_bound), -1)
        margin = f32(1.0) - f32(2.0 ** -18)
        held = np.zeros(0, u64)
        r = 0
        with np.errstate(all="ignore"):
            while True:
                new = keys[(upto[r - 1] if r else 0):upto[r]]
                new = new[new <= bound_key]                      # (take: key <= bound_key && key < worst)
                if len(new):
                    held = np.sort(np.concatenate([held, new]))
                    if k is not None:
                        held = held[:k]
                worst = held[k - 1] if k is not None and len(held) == k else KEY_INF
                if f32(lb[r] * margin) > np.fmin(key_d2(worst), f32(d2_bound)) or r == rmax:      # walk_done
                    break
                r += 1
        return held, int(upto[r]), r

    def many(self, Q, k, max_distance=np.inf, slack=True):
        """Every query of Q -> (index (m, k) int32, distance (m, k) f32, found (m,), candidates (m,), last shell (m,)); the slots
        beyond `found` hold -1 and FLT_MAX as the library's do.  k None: the radius query as (offsets, index, distance, candidates,
        last shell)."""
        Q = np.asarray(Q, f32).reshape(-1, 3)
        bound = radius_d2_bound(max_distance)
        rows = [self.query(q, k, bound, slack) for q in Q]
        cand = np.array([r[1] for r in rows], np.int64)
        last = np.array([r[2] for r in rows], np.int64)
        if k is None:
            off = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
            keys = np.concatenate([r[0] for r in rows] + [np.zeros(0, u64)])
            return off, key_index(keys), sqrt_rn(key_d2(keys)), cand, last
        idx = np.full((len(Q), k), -1, np.int32)
        dist = np.full((len(Q), k), FLT_MAX, f32)
        found = np.zeros(len(Q), np.int32)
        for i, (keys, _, _) in enumerate(rows):
            idx[i, :len(keys)] = key_index(keys)
            dist[i, :len(keys)] = sqrt_rn(key_d2(keys))
            found[i] = len(keys)
        return idx, dist, found, cand, last


# ---- queries --------------------------------------------------------------------------------------------------------------
N_NEAR = 130


def queries_for(P, seed, n_jitter=90, n_static=N_NEAR - 90, per_axis=4):
    """What every case is asked: static points jittered by about half a cell; static points themselves; the f32 cell boundaries of
    the cloud's grid and their two f32 neighbours along each axis (the other coordinates inside the box); the corners and face
    centres of the box; meshsdf_cases.outside_queries' directions at 10, 1000 and 10^6 extents."""
    P = np.asarray(P, f32).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    G = cloud_grid(P)
    lo, hi = P.min(0).astype(f64), P.max(0).astype(f64)
    with np.errstate(all="ignore"):
        jitter = (P[rng.integers(0, len(P), n_jitter)].astype(f64) + rng.normal(0, 0.5, (n_jitter, 3)) * f64(G["h"])).astype(f32)
        own = P[rng.integers(0, len(P), n_static)]
        edges = []
        for a in range(3):
            if G["dim"][a] < 2:
                continue
            for c in np.unique(rng.integers(1, G["dim"][a], per_axis)):
                bf = boundary(G, a, c)
                for x in (np.nextafter(bf, f32(-np.inf)), bf, np.nextafter(bf, f32(np.inf))):
                    p = (lo + rng.random(3) * (hi - lo)).astype(f32)
                    p[a] = x
                    edges.append(p)
        outside = MC.outside_queries(P, np.arange(len(P)))
    return np.ascontiguousarray(np.concatenate([jitter, own, np.array(edges, f32).reshape(-1, 3), outside]).astype(f32))


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def base_cloud(seed=201):
    """N_POINTS uniform in [-1, 1]^3."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (N_POINTS, 3)).astype(f32)


def unit_cube(seed=202):
    """N_POINTS uniform in the unit cube about the origin, binary64 (the far cases translate it before rounding)."""
    return np.random.default_rng(seed).random((N_POINTS, 3)) - 0.5


def needle(length=100.0, radius=0.5, seed=203):
    rng = np.random.default_rng(seed)
    ang, rad = rng.uniform(0, 2 * np.pi, N_POINTS), radius * np.sqrt(rng.random(N_POINTS))
    return np.stack([rng.uniform(0, length, N_POINTS), rad * np.cos(ang), rad * np.sin(ang)], 1).astype(f32)


def sheet(thickness=1e-3, seed=204):
    rng = np.random.default_rng(seed)
    return (rng.random((N_POINTS, 3)) * [1.0, 1.0, thickness]).astype(f32)


def two_clusters(gap=40.0, seed=205):
    """Two balls of diameter 1, N_POINTS / 2 points each, their centres `gap` diameters apart along x."""
    rng = np.random.default_rng(seed)
    blobs = []
    for cx in (0.0, gap):
        d = rng.normal(size=(N_POINTS // 2, 3))
        d *= (0.5 * rng.random((N_POINTS // 2, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        blobs.append(d + [cx, 0.0, 0.0])
    return np.concatenate(blobs).astype(f32)


def cluster_queries(gap=40.0, seed=206):
    """In the void between the clusters, beside each of them, and beyond each of them."""
    rng = np.random.default_rng(seed)
    void = np.stack([rng.uniform(1.0, gap - 1.0, 60), rng.uniform(-1.5, 1.5, 60), rng.uniform(-1.5, 1.5, 60)], 1)
    mid = np.array([[gap / 2, 0, 0], [gap / 2, 0.25, -0.125], [gap / 2 - 0.5, 0, 0], [gap / 2 + 0.5, 0, 0]])
    beside = np.concatenate([np.stack([rng.uniform(-0.7, 0.7, 20) + cx, rng.uniform(-3, 3, 20), rng.uniform(-3, 3, 20)], 1) for cx in (0.0, gap)])
    far = np.concatenate([np.stack([cx + sg * rng.uniform(0.6, 30, 15), rng.uniform(-2, 2, 15), rng.uniform(-2, 2, 15)], 1)
                          for cx, sg in ((0.0, -1.0), (gap, 1.0))])
    return np.concatenate([void, mid, beside, far]).astype(f32)


# ---- traps ----------------------------------------------------------------------------------------------------------------
def boundary_traps(P, scale=1.0, want=12, seed=207):
    """meshsdf_cases.boundary_traps carried over to points: replaces 2 * want points of the cloud P (its box, count and so its
    grid unchanged) by pairs that only the slack of the shell bound keeps apart.  A trap sits at a cell boundary c along one axis
    whose f32 position in the shell bound, bf = lo + (float)c * h, lies a few f32 steps ABOVE coordinates that cell_of still puts
    into cell c: a lone point at such a coordinate x1 < bf (in cell c); the query at bf - g in cell c - 1; a second point in cell
    c - 1 on the query's other side at a distance D with g - (bf - x1) < D < g (1 - 2^-19).  The first is the nearest point, and
    the second is within the bound that a walk without slack computes for cell c (g^2 (1 - 2^-18)): such a walk stops at the
    second.  The other coordinates are mid-cell, and the background is redrawn away from the traps.  scale: the power of two P was
    multiplied with (g follows it).  Returns (P, queries, winners)."""
    rng = np.random.default_rng(seed)
    P = np.array(P, f32).reshape(-1, 3).copy()
    G = cloud_grid(P)
    n = len(P)
    lo, hi = P.min(0), P.max(0)
    corner = np.nonzero(((P == lo[None]) | (P == hi[None])).any(axis=1))[0]      # (the points that make the box stay)
    g = 0.002 * scale
    queries, winners = [], []
    held = set(corner.tolist())
    free = [i for i in range(n) if i not in held]
    for a in (2, 1, 0):
        for c in range(1, G["dim"][a]):
            if len(queries) >= want:
                break
            bf = boundary(G, a, c)
            x1, steps = bf, 0
            while True:      # the lowest coordinate below bf that cell_of still puts into cell c
                nx = np.nextafter(x1, f32(-np.inf))
                p = G["lo"].copy()
                p[a] = nx
                if cell_of(G, p[None])[0, a] != c:
                    break
                x1, steps = nx, steps + 1
            if steps < 2:
                continue
            qa = f32(f64(bf) - g)
            d1 = f64(x1) - f64(qa)                                   # the distance of the first point
            bound = f64(f32(bf - qa)) * (1.0 - 2.0 ** -19)           # below it, the second is within the slack-free bound of cell c
            x2 = f32(f64(qa) - 0.5 * (d1 + bound))
            D = f64(qa) - f64(x2)
            if not (d1 < D < bound):
                continue
            centre = G["lo"].astype(f64) + (rng.integers(2, np.array(G["dim"]) - 2) + 0.5) * f64(G["h"])   # mid-cell on the other axes
            q, p1, p2 = centre.copy(), centre.copy(), centre.copy()
            q[a], p1[a], p2[a] = qa, x1, x2
            first, second = free[len(queries)], free[-1 - len(queries)]
            P[first], P[second] = p1.astype(f32), p2.astype(f32)
            queries.append(q.astype(f32))
            winners.append(first)
    Q = np.array(queries, f32).reshape(-1, 3)
    W = np.array(winners, np.int64)
    # the background: no other point within a third of a cell of a trap's query
    trap = np.zeros(n, bool)
    trap[W] = True
    trap[[free[-1 - i] for i in range(len(W))]] = True
    trap[corner] = True
    for _ in range(100):
        near = (np.abs(P[:, None, :].astype(f64) - Q[None].astype(f64)).max(axis=2) < f64(G["h"]) / 3).any(axis=1) & ~trap
        if not near.any():
            break
        P[near] = (lo.astype(f64) + rng.random((int(near.sum()), 3)) * (hi.astype(f64) - lo.astype(f64))).astype(f32)
    assert not near.any() and (P.min(0) == lo).all() and (P.max(0) == hi).all()
    return np.ascontiguousarray(P), Q, W.astype(np.int32)


# ---- the cases ------------------------------------------------------------------------------------------------------------
TRAP_SCALES = (0, -40, 40)                       # binary exponents
FAR = {"far4096": 4096.0, "far65536": 65536.0, "far2p20": 2.0 ** 20}
SCALES = (-66, -70, -75, -140, 63, 64, 100)
# (exponents at which everything scales exactly are not cases of their own: test_points_walk_model.py compares them with "base")
NAMES = ("base", "cube") + tuple(f"traps_{e}" for e in TRAP_SCALES) + tuple(FAR) + tuple(f"scale_{e}" for e in SCALES) + \
    ("needle", "sheet", "two_clusters")

_made = {}


def scaled(A, e):
    """A * 2^e in f32, in two exact halves (2^e itself is no f32 at e = -140): exact unless the result leaves the normal range."""
    half = f32(2.0) ** f32(e // 2)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray((np.asarray(A, f32) * half) * (f32(2.0) ** f32(e - e // 2)))


def case(name):
    """name -> (static points (n, 3) f32, queries (m, 3) f32), made once and read-only.  traps_<e>: the trap queries come first
    (trap_queries(name) tells how many, and the winners).  near_queries(name): the slice of the queries at and about static points."""
    if name in _made:
        return _made[name][:2]
    extra, first = None, 0
    if name == "base":
        P = base_cloud()
        Q = queries_for(P, 301)
    elif name == "cube":
        P = unit_cube().astype(f32)
        Q = queries_for(P, 302)
    elif name.startswith("traps_"):
        e = int(name[6:])
        P, tq, winners = boundary_traps(scaled(base_cloud(), e), 2.0 ** e)
        Q = np.concatenate([tq, queries_for(P, 303)])
        extra, first = (len(tq), winners), len(tq)
    elif name in FAR:
        P = (unit_cube() + FAR[name]).astype(f32)
        Q = queries_for(P, 304)
    elif name.startswith("scale_"):
        e = int(name[6:])
        B, BQ = case("base")
        P, Q = scaled(B, e), scaled(BQ, e)
    elif name == "needle":
        P = needle()
        Q = queries_for(P, 305)
    elif name == "sheet":
        P = sheet()
        Q = queries_for(P, 306)
    elif name == "two_clusters":
        P = two_clusters()
        Q = np.concatenate([queries_for(P, 307), cluster_queries()])
    else:
        raise KeyError(name)
    P, Q = np.ascontiguousarray(P, f32), np.ascontiguousarray(Q, f32)
    assert len(P) <= N_POINTS and len(Q) <= 400, (name, len(P), len(Q))
    P.setflags(write=False)
    Q.setflags(write=False)
    _made[name] = (P, Q, extra, slice(first, first + N_NEAR))
    return P, Q


def trap_queries(name):
    """-> (number of trap queries at the head of the case's queries, the static point each of them has to find)."""
    case(name)
    return _made[name][2]


def near_queries(name):
    """The slice of the case's queries that a scan would ask: the jittered static points and the static points themselves."""
    case(name)
    return _made[name][3]


def radius_of(name):
    """The radius the tests ask each case with: about two cells of its grid."""
    with np.errstate(all="ignore"):
        return f32(f32(2) * cloud_grid(case(name)[0])["h"])


_walks, _answers = {}, {}


def walk_of(name):
    if name not in _walks:
        _walks[name] = Walk(case(name)[0])
    return _walks[name]


def answers(name, k, max_distance=np.inf, slack=True):
    """Walk.many of the case's queries, computed once and shared (read-only)."""
    key = (name, k, float(max_distance), slack)
    if key not in _answers:
        out = walk_of(name).many(case(name)[1], k, max_distance, slack)
        for a in out:
            a.setflags(write=False)
        _answers[key] = out
    return _answers[key]


def summary(names=NAMES):
    """What tests/golden/points_walk_cases.json records of every case: the sizes, the grid, and for the nearest point (k = 1) and
    k = 8 the candidates over all queries, those of the queries at and about static points (near_queries: what a scan asks; per
    query too), and the last shells walked (their sum and mean over the finite queries).  Counts of the model, not times."""
    out = {}
    for name in names:
        P, Q = case(name)
        G = walk_of(name).G
        row = {"points": len(P), "distinct_points": int(len(np.unique(P, axis=0))), "queries": len(Q),
               "finite_queries": int(np.isfinite(Q).all(axis=1).sum()), "grid": [int(d) for d in G["dim"]]}
        for k in (1, 8):
            _, _, _, cand, last = answers(name, k)
            walked = last[last >= 0]
            near = cand[near_queries(name)]
            row[f"k{k}"] = {"candidates": int(cand.sum()), "near_candidates": int(near.sum()), "near_candidates_per_query": float(near.sum() / len(near)),
                            "last_shell_sum": int(walked.sum()), "mean_last_shell": float(walked.sum() / max(1, len(walked)))}
        out[name] = row
    return out
