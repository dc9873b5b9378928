"""numpy model of Voxels.Redistance (include/sdfkit_hip.h, "Redistancing"; the arithmetic of sdfkit_amd/csrc/redistance.h): the
five steps of the contract, vectorised, binary64 in the header's operation order, full Jacobi sweeps to the fixed point.  The
authority the host solver and the GPU are compared with, bit for bit.

The only shortcut is exact: a sweep is evaluated on the bounding box of the finite values grown by one voxel (a voxel at +inf
whose six neighbours are at +inf stays there)."""
import numpy as np

f32, f64 = np.float32, np.float64
TILE = 8


def cell_sizes(mn, mx, shape):
    """(DX, DY, DZ) as the library computes them: f32 (max - min) / n."""
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    return np.array([f32(f32(mx[a] - mn[a]) / f32(shape[a])) for a in range(3)], f32)


def _shift(s, a, side):
    """(neighbour values at x - e_a (side 0) / x + e_a (side 1), in-range mask)"""
    n = np.roll(s, 1 if side == 0 else -1, axis=a)
    idx = np.arange(s.shape[a])
    ok = (idx > 0) if side == 0 else (idx < s.shape[a] - 1)
    shape = [1, 1, 1]
    shape[a] = -1
    return n, np.broadcast_to(ok.reshape(shape), s.shape)


def front(values, h, iso=0.0):
    """Step 2 -> (outside bool, frozen bool, T0 f32 with +inf off the front)."""
    s = np.asarray(values, f32).astype(f64) - f64(f32(iso))
    h = np.asarray(h, f32).astype(f64)
    out = s > 0.0
    mag = np.abs(s)
    q = np.zeros(s.shape, f64)
    frozen = np.zeros(s.shape, bool)
    zero = np.zeros(s.shape, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            t = np.full(s.shape, np.inf)
            has = np.zeros(s.shape, bool)
            for side in (0, 1):
                sn, ok = _shift(s, a, side)
                cross = ok & ((sn > 0.0) != out)
                c = (h[a] * mag) / (mag + np.abs(sn))
                t = np.where(cross & (~has | (c < t)), c, t)
                has |= cross
            frozen |= has
            zero |= has & (t == 0.0)
            q = q + np.where(has, 1.0 / (t * t), 0.0)
        t0 = np.where(zero, 0.0, 1.0 / np.sqrt(q)).astype(f32)
    return out, frozen, np.where(frozen, t0, f32(np.inf)).astype(f32)


def update(a, h):
    """Step 3's u as f32 from a (3, ...) binary64 upwind values and the three cell sizes (binary64)."""
    order = np.argsort(a, axis=0, kind="stable")
    a = np.take_along_axis(a, order, 0)
    hs = np.asarray(h, f64)[order]
    with np.errstate(all="ignore"):
        w = 1.0 / (hs * hs)
        u = a[0] + hs[0]
        A = w[0] + w[1]
        B = w[0] * a[0] + w[1] * a[1]
        S = (w[0] * a[0]) * a[0] + (w[1] * a[1]) * a[1]
        D = B * B - A * (S - 1.0)
        two = u > a[1]
        u = np.where(two, (B + np.sqrt(np.where(D > 0.0, D, 0.0))) / A, u)
        A = A + w[2]
        B = B + w[2] * a[2]
        S = S + (w[2] * a[2]) * a[2]
        D = B * B - A * (S - 1.0)
        three = two & (u > a[2])
        u = np.where(three, (B + np.sqrt(np.where(D > 0.0, D, 0.0))) / A, u)
        return u.astype(f32)


def sweep(T, frozen, h, band=np.inf):
    """One Jacobi sweep: T_k -> T_k+1 (a new array)."""
    h = np.asarray(h, f32).astype(f64)
    fin = np.nonzero(np.isfinite(T))
    new = T.copy()
    if len(fin[0]) == 0:
        return new
    lo = [max(int(i.min()) - 1, 0) for i in fin]
    hi = [min(int(i.max()) + 2, n) for i, n in zip(fin, T.shape)]
    P = np.pad(T, 1, constant_values=np.inf)
    box = tuple(slice(l, u) for l, u in zip(lo, hi))

    def nb(a, d):   # T(x + d e_a) on the box, from the padded array
        return P[tuple(slice(l + 1 + (d if k == a else 0), u + 1 + (d if k == a else 0)) for k, (l, u) in enumerate(zip(lo, hi)))]
    a = np.stack([np.where(nb(k, -1) < nb(k, 1), nb(k, -1), nb(k, 1)).astype(f64) for k in range(3)])
    uf = update(a, h)
    t = T[box]
    new[box] = np.where(~frozen[box] & (uf < t) & (uf <= f32(band)), uf, t)
    return new


def _tiles_of(mask):
    pad = [(0, (-n) % TILE) for n in mask.shape]
    m = np.pad(mask, pad)
    tx, ty, tz = (n // TILE for n in m.shape)
    return m.reshape(tx, TILE, ty, TILE, tz, TILE).any(axis=(1, 3, 5))


def _dilate6(t):
    out = t.copy()
    for a in range(3):
        sl_lo = [slice(None)] * 3
        sl_hi = [slice(None)] * 3
        sl_lo[a], sl_hi[a] = slice(0, -1), slice(1, None)
        out[tuple(sl_lo)] |= t[tuple(sl_hi)]
        out[tuple(sl_hi)] |= t[tuple(sl_lo)]
    return out


def redistance(values, h, iso=0.0, max_distance=np.inf, max_sweeps=None, history=None):
    """Steps 2-5 -> (result f32, stats): stats = sweeps (the last, which changes nothing, included; 0 without a front),
    tile_sweeps (8^3 tiles the block-active schedule sweeps), front voxels, clamped voxels (T > max_distance).
    history: a list that receives, per sweep, (the mask of tiles the schedule sweeps, the mask of tiles the sweep changed)."""
    values = np.asarray(values, f32)
    if not np.all(np.isfinite(values)) or not np.isfinite(f32(iso)) or not (f32(max_distance) >= 0):
        raise ValueError("refused (step 1)")
    hf = np.asarray(h, f32)
    if hf.shape != (3,) or not np.all(np.isfinite(hf)) or not np.all(hf > 0):
        raise ValueError("refused (step 1): cell sizes %r are not finite and > 0" % (hf.tolist(),))
    band = f32(max_distance)
    out, frozen, T = front(values, h, iso)
    sweeps = tile_sweeps = 0
    if frozen.any():
        changed_tiles = _tiles_of(frozen)
        while max_sweeps is None or sweeps < max_sweeps:
            new = sweep(T, frozen, h, band)
            sweeps += 1
            swept = _dilate6(changed_tiles)
            tile_sweeps += int(swept.sum())
            changed = new != T
            if history is not None:
                history.append((swept, _tiles_of(changed)))
            if not changed.any():
                break
            changed_tiles = _tiles_of(changed)
            T = new
    m = np.where(T < band, T, band).astype(f32)
    res = np.where(out, m, -m).astype(f32)
    stats = {"sweeps": sweeps, "tile_sweeps": tile_sweeps, "front": int(frozen.sum()), "clamped": int((T > band).sum())}
    return res, stats


# ---- the block-active schedule, sweep by sweep (tests/redistance_cases.py) -------------------------------------------------------
def schedule_history(values, h, iso=0.0, band=np.inf, changes=False):
    """Per sweep, the boolean mask of the 8^3 tiles the schedule of redistance() sweeps (their sum is stats["tile_sweeps"]).
    changes=True: (those masks, per sweep the mask of tiles in which the sweep changed a value)."""
    hist = []
    redistance(values, h, iso, band, history=hist)
    swept, changed = [s for s, _ in hist], [c for _, c in hist]
    return (swept, changed) if changes else swept


def idle_runs(history):
    """[(tile index, first sweep of the gap (0-based), gap length g >= 1)]: the tile is swept in sweep first - 1, not swept in the
    g sweeps from `first` on, and swept again in sweep first + g."""
    runs = []
    if not history:
        return runs
    H = np.stack(history)   # (sweeps, tx, ty, tz)
    for tile in np.argwhere(H.any(axis=0)):
        col = H[(slice(None),) + tuple(tile)]
        on = np.flatnonzero(col)
        for a, b in zip(on[:-1], on[1:]):
            if b - a > 1:
                runs.append((tuple(int(t) for t in tile), int(a) + 1, int(b - a - 1)))
    return runs


def idle_gaps(history):
    """The set of gap lengths g >= 1: runs of g sweeps in which a tile is not swept, between two sweeps in which it is."""
    return {g for _, _, g in idle_runs(history)}


# ---- the cases the tests and tools/gen_redistance_accuracy.py share --------------------------------------------------------------
def centres(mn, mx, shape):
    """Cell centres as the library places them (f32: min + size / n / 2, then + k size / n), as three broadcastable f64 arrays."""
    d = cell_sizes(mn, mx, shape)
    mn = np.asarray(mn, f32)
    ax = []
    for a in range(3):
        first = f32(mn[a] + f32(f32(0.5) * d[a]))
        ax.append((first + np.arange(shape[a], dtype=f32) * d[a]).astype(f32).astype(f64))
    return np.meshgrid(*ax, indexing="ij")


def sphere_inputs(n, kind, r=1.0, half=1.5):
    """The issue's sphere r = 1 in [-1.5, 1.5]^3 at n^3 as (a) its exact distance, (b) 3 (|p| - 1), (c) |p|^2 - 1
    -> (values f32, h, exact distance f64)."""
    mn, mx = [-half] * 3, [half] * 3
    x, y, z = centres(mn, mx, (n, n, n))
    rad = np.sqrt(x * x + y * y + z * z)
    d = rad - r
    v = {"a": d, "b": 3.0 * d, "c": rad * rad - r * r}[kind]
    return v.astype(f32), cell_sizes(mn, mx, (n, n, n)), d


# ---- the g++ host solver of tests/cpp/redistance_host.cpp (csrc/redistance.h, full sweeps) --------------------------------------
def build_host_solver(out_dir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(out_dir), "redistance_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", os.path.join(root, "tests", "cpp", "redistance_host.cpp"),
                           "-o", exe])
    return exe


def host_solve(exe, values, h, iso, max_distance, tmp_dir, tag="case", timeout=900):
    """-> (result f32, stats dict without tile_sweeps)"""
    import os
    import subprocess
    values = np.ascontiguousarray(values, f32)
    src, dst = os.path.join(str(tmp_dir), tag + ".in"), os.path.join(str(tmp_dir), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.asarray(values.shape, np.int32).tobytes())
        f.write(np.asarray(list(h) + [iso, max_distance], f32).tobytes())
        f.write(values.tobytes())
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0 and "redistance ok" in p.stdout, (p.returncode, p.stderr)
    raw = np.fromfile(dst, np.uint8)
    res = raw[: values.size * 4].view(f32).reshape(values.shape)
    st = raw[values.size * 4:].view(np.int64)
    return res, {"sweeps": int(st[0]), "front": int(st[2]), "clamped": int(st[3])}


# ---- the measurements of tests/golden/redistance_accuracy.json (tools/gen_redistance_accuracy.py, tests/test_redistance_model.py) --
def edge_crossing_shift(values, result, iso=0.0):
    """Max over the sign-changing grid edges of |crossing of the result - crossing of the input| in units of the edge, both placed
    by linear interpolation as marching cubes does."""
    s = np.asarray(values, f32).astype(f64) - f64(f32(iso))
    o = np.asarray(result, f32).astype(f64)
    worst = 0.0
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        s0, s1, o0, o1 = s[tuple(lo)], s[tuple(hi)], o[tuple(lo)], o[tuple(hi)]
        cross = (s0 > 0) != (s1 > 0)
        with np.errstate(all="ignore"):
            ti = np.abs(s0) / (np.abs(s0) + np.abs(s1))
            to = np.abs(o0) / (np.abs(o0) + np.abs(o1))
        if cross.any():
            worst = max(worst, float(np.max(np.abs(ti - to)[cross])))
    return worst


def sphere_record(n, kind):
    v, h, d = sphere_inputs(n, kind)
    out, st = redistance(v, h)
    dx = float(h[0])
    err = np.abs(out.astype(f64) - d) / dx
    before = np.abs(v.astype(f64) - d) / dx
    return {"max": float(err.max()), "mean": float(err.mean()), "input_max": float(before.max()), "input_mean": float(before.mean()),
            "sweeps": st["sweeps"], "front": st["front"], "edge_shift": edge_crossing_shift(v, out)}


def mesh_case(name, n=16):
    """A box and the union of two spheres on [-1.5, 1.5]^3 (scaled by 2: not a distance) -> (values f32, mn, mx)."""
    mn, mx = [-1.5] * 3, [1.5] * 3
    x, y, z = centres(mn, mx, (n, n, n))
    if name == "box":
        q = [np.abs(c) - b for c, b in zip((x, y, z), (0.9, 0.6, 0.75))]
        d = np.sqrt(sum(np.maximum(c, 0.0) ** 2 for c in q)) + np.minimum(np.maximum(np.maximum(q[0], q[1]), q[2]), 0.0)
    else:
        d = np.minimum(np.sqrt((x + 0.4) ** 2 + y * y + z * z) - 0.7, np.sqrt((x - 0.5) ** 2 + (y - 0.2) ** 2 + (z + 0.1) ** 2) - 0.55)
    return (2.0 * d).astype(f32), mn, mx


def mesh_record(name, n=16):
    """|result| against the exact distance to the marching-cubes mesh of the input (oracle march + meshsdf_model.closest)."""
    from oracle import oracle as O
    from tests import meshsdf_model as MS
    v, mn, mx = mesh_case(name, n)
    h = cell_sizes(mn, mx, v.shape)
    out, st = redistance(v, h)
    mesh = O.march(v, None, mn, mx, 0.0)
    x, y, z = centres(mn, mx, v.shape)
    Q = np.stack([x, y, z], -1).reshape(-1, 3).astype(f32)
    _, _, _, _, d2 = MS.closest(mesh.vertices, mesh.triangles, Q)
    exact = np.sqrt(d2).reshape(v.shape)
    dx = float(h[0])
    err = np.abs(np.abs(out.astype(f64)) - exact) / dx
    before = np.abs(np.abs(v.astype(f64)) - exact) / dx
    return {"n": n, "max": float(err.max()), "mean": float(err.mean()), "input_max": float(before.max()), "input_mean": float(before.mean()),
            "sweeps": st["sweeps"], "triangles": int(len(mesh.triangles) // 3), "edge_shift": edge_crossing_shift(v, out)}
