"""numpy float32 model of the volume-reading SDF operations (include/sdfkit_hip.h: SDFK_OP_VOXEL_NEAREST / SDFK_OP_VOXEL_LINEAR),
of whole programs that use them (every other opcode evaluated as oracle/ir_interp.py does, with its helpers), of the grid sampler's
points, of the ray marcher's per-pixel arithmetic, and of the min/max pyramid bound the block culling reads.

A volume here is a tuple (values [nx, ny, nz], colors [nx, ny, nz, 3] or None, min[3], max[3]), float32."""
import numpy as np

from oracle import ir_interp as I

f32 = np.float32
NEAREST, LINEAR = 17, 18


def vol_d(vol):
    vals, _, mn, mx = vol
    n = np.array(vals.shape, f32)
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    return (mx - mn) / n   # Voxels.cs:32-34


def _channel(vol, ch):
    vals, cols, _, _ = vol
    return vals if ch == 3 else cols[..., ch]


def near_idx(q, n):
    """clamped truncation of quotients q (not NaN) to [0, n - 1]"""
    with np.errstate(invalid="ignore"):
        i = np.where(q > 0, np.where(q < f32(n - 1), np.trunc(np.where(np.isfinite(q), q, 0)), n - 1), 0)
    return np.minimum(i.astype(np.int64), n - 1)


def quot(X, mn, d):
    with np.errstate(all="ignore"):
        return ((np.asarray(X, f32) - f32(mn)).astype(f32) / f32(d)).astype(f32)


def nearest(vol, ch, X, Y, Z):
    mn = np.asarray(vol[2], f32)
    d = vol_d(vol)
    data = _channel(vol, ch)
    q = [quot(c, mn[a], d[a]) for a, c in enumerate((X, Y, Z))]
    bad = np.isnan(q[0]) | np.isnan(q[1]) | np.isnan(q[2])
    idx = [near_idx(np.where(np.isnan(qa), f32(0), qa), data.shape[a]) for a, qa in enumerate(q)]
    return np.where(bad, f32(np.nan), data[idx[0], idx[1], idx[2]]).astype(f32)


def lin_u(X, m, d, n):
    u = quot(X, m, d)
    u = np.where(u > 0, u, f32(0)).astype(f32)
    top = f32(n - 1)
    return np.where(u < top, u, top).astype(f32)


def lin_i0(u, n):
    if n == 1:
        return np.zeros(u.shape, np.int64)
    with np.errstate(invalid="ignore"):
        i = np.floor(np.where(np.isfinite(u), u, 0)).astype(np.int64)
    return np.minimum(i, n - 2)


def _lerp(a, b, f):
    with np.errstate(all="ignore"):
        return (a + (f * (b - a)).astype(f32)).astype(f32)


def linear(vol, ch, X, Y, Z):
    vals = vol[0]
    n = vals.shape
    d = vol_d(vol)
    mn = np.asarray(vol[2], f32)
    m = (mn + (f32(0.5) * d).astype(f32)).astype(f32)
    X, Y, Z = (np.asarray(c, f32) for c in (X, Y, Z))
    bad = np.isnan(X) | np.isnan(Y) | np.isnan(Z)
    u = [lin_u(np.where(bad, f32(0), c), m[a], d[a], n[a]) for a, c in enumerate((X, Y, Z))]
    i0 = [lin_i0(u[a], n[a]) for a in range(3)]
    i1 = [i0[a] + 1 if n[a] > 1 else i0[a] for a in range(3)]
    f = [(u[a] - i0[a].astype(f32)).astype(f32) if n[a] > 1 else np.zeros(u[a].shape, f32) for a in range(3)]
    data = _channel(vol, ch)
    c = {}
    for k in range(8):
        ix = i1[0] if k & 1 else i0[0]
        iy = i1[1] if k & 2 else i0[1]
        iz = i1[2] if k & 4 else i0[2]
        c[k] = data[ix, iy, iz]
    a00, a10 = _lerp(c[0], c[1], f[0]), _lerp(c[2], c[3], f[0])
    a01, a11 = _lerp(c[4], c[5], f[0]), _lerp(c[6], c[7], f[0])
    b0, b1 = _lerp(a00, a10, f[1]), _lerp(a01, a11, f[1])
    r = _lerp(b0, b1, f[2])
    mi, ma = I._min_ieee, I._max_ieee
    lo = mi(mi(mi(c[0], c[1]), mi(c[2], c[3])), mi(mi(c[4], c[5]), mi(c[6], c[7])))
    hi = ma(ma(ma(c[0], c[1]), ma(c[2], c[3])), ma(ma(c[4], c[5]), ma(c[6], c[7])))
    with np.errstate(invalid="ignore"):
        r = np.where(r >= lo, np.where(r <= hi, r, hi), lo)
    return np.where(bad, f32(np.nan), r).astype(f32)


def _eval(ops, px, py, pz, volumes):
    """every value of the program at the points, ir_interp's semantics plus the two volume reads"""
    v = []
    with np.errstate(all="ignore"):
        for (op, a, b, c, dd, imm) in ops:
            if op in (NEAREST, LINEAR):
                fn = nearest if op == NEAREST else linear
                r = fn(volumes[dd >> 2], dd & 3, v[a], v[b], v[c])
            elif op == I.CONST: r = np.full(px.shape, f32(imm), f32)
            elif op == I.X: r = px
            elif op == I.Y: r = py
            elif op == I.Z: r = pz
            elif op == I.ADD: r = v[a] + v[b]
            elif op == I.SUB: r = v[a] - v[b]
            elif op == I.MUL: r = v[a] * v[b]
            elif op == I.DIV: r = v[a] / v[b]
            elif op == I.NEG: r = -v[a]
            elif op == I.ABS: r = np.abs(v[a])
            elif op == I.SQRT: r = np.sqrt(v[a])
            elif op == I.FLOOR: r = np.floor(v[a])
            elif op == I.MIN_SEL: r = np.where(v[a] < v[b], v[a], v[b])
            elif op == I.MAX_SEL: r = np.where(v[a] > v[b], v[a], v[b])
            elif op == I.MIN_IEEE: r = I._min_ieee(v[a], v[b])
            elif op == I.MAX_IEEE: r = I._max_ieee(v[a], v[b])
            elif op == I.SEL_LT: r = np.where(v[a] < v[b], v[c], v[dd])
            else: raise ValueError(op)
            v.append(np.asarray(r, f32))
    return v


def run(ops, out_rgbw, points, volumes):
    """the program at points [n, 3]: [r, g, b, w] (None for an output id < 0)"""
    pts = np.asarray(points, f32)
    v = _eval(ops, np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1]), np.ascontiguousarray(pts[:, 2]), volumes)
    return [v[k] if k >= 0 else None for k in out_rgbw]


def grid_points(mn, mx, nx, ny, nz):
    """Voxels.SampleSdf's sample points (Voxels.cs:81,104-106), [nx, ny, nz] arrays"""
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    d = (mx - mn) / np.array([nx, ny, nz], f32)
    m = mn + f32(0.5) * d
    px = (m[0] + np.arange(nx, dtype=f32) * d[0])[:, None, None] + np.zeros((nx, ny, nz), f32)
    py = (m[1] + np.arange(ny, dtype=f32) * d[1])[None, :, None] + np.zeros((nx, ny, nz), f32)
    pz = (m[2] + np.arange(nz, dtype=f32) * d[2])[None, None, :] + np.zeros((nx, ny, nz), f32)
    return px, py, pz


def sample(ops, out_rgbw, writes_color, mn, mx, nx, ny, nz, volumes, clip=False):
    """Voxels.SampleSdf (+ ClipToBounds) of a program: (values, colors)"""
    px, py, pz = grid_points(mn, mx, nx, ny, nz)
    v = _eval(ops, px, py, pz, volumes)
    values = v[out_rgbw[3]].copy()
    colors = np.stack([v[out_rgbw[k]] for k in range(3)], -1) if writes_color else np.zeros((nx, ny, nz, 3), f32)
    if clip:   # Voxels.cs:133-167: the outer wall becomes DX
        outside = f32((f32(mx[0]) - f32(mn[0])) / f32(nx))
        values[0], values[-1], values[:, 0], values[:, -1], values[:, :, 0], values[:, :, -1] = (outside,) * 6
    return values, colors


def raymarch(ops, out_rgbw, writes_color, volumes, width, height, cam, m, nearp, farp, iters):
    """sdfk_raymarch's per-pixel arithmetic (csrc/sample_codegen.h), op for op in float32: (depth [h, w], rgb [h, w, 3])"""
    with np.errstate(all="ignore"):
        k = np.arange(width * height)
        j, i = k // width, k % width
        y = (f32(1) - (f32(2) * j.astype(f32)).astype(f32) / f32(height - 1)).astype(f32)
        x = (f32(-1) + (f32(2) * i.astype(f32)).astype(f32) / f32(width - 1)).astype(f32)
        m = np.asarray(m, f32).reshape(-1)
        cam = np.asarray(cam, f32).reshape(-1)
        v4 = [(((x * m[q]).astype(f32) + (y * m[4 + q]).astype(f32)).astype(f32) + (f32(0) * m[8 + q]).astype(f32) + (f32(1) * m[12 + q])).astype(f32)
              for q in range(4)]
        dx, dy, dz = ((v4[a] / v4[3]).astype(f32) - cam[a] for a in range(3))
        dl = np.sqrt((((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)).astype(f32))
        rx, ry, rz = dx / dl, dy / dl, dz / dl
        depth = np.full(k.shape, f32(nearp) - f32(0.1), f32)
        cr = cg = cb = np.zeros(k.shape, f32)

        def scene(px, py, pz):
            r = run(ops, out_rgbw, np.stack([px, py, pz], -1), volumes)
            z = np.zeros(px.shape, f32)
            return (r[0], r[1], r[2], r[3]) if writes_color else (z, z, z, r[3])
        for _ in range(iters):
            cr, cg, cb, w = scene((rx * depth).astype(f32) + cam[0], (ry * depth).astype(f32) + cam[1], (rz * depth).astype(f32) + cam[2])
            depth = (depth + w).astype(f32)
        d0, d1, d2 = (f32(0) + cr, f32(0) + cg, f32(0) + cb) if iters > 0 else (np.zeros(k.shape, f32),) * 3
        sx, sy, sz = (cam[0] + (rx * depth).astype(f32)).astype(f32), (cam[1] + (ry * depth).astype(f32)).astype(f32), (cam[2] + (rz * depth).astype(f32)).astype(f32)
        go = f32(1e-5)
        ws = []
        for sgn in (go, -go):
            for ax in range(3):
                e = [f32(1.0) if a == ax else f32(0.0) for a in range(3)]
                ws.append(scene((sx + (sgn * e[0])).astype(f32), (sy + (sgn * e[1])).astype(f32), (sz + (sgn * e[2])).astype(f32))[3])
        nx, ny, nz = ws[0] - ws[3], ws[1] - ws[4], ws[2] - ws[5]

        def normalize(a, b, c):
            ln = np.sqrt((((a * a).astype(f32) + (b * b).astype(f32)).astype(f32) + (c * c).astype(f32)).astype(f32))
            r = (f32(1) / ln).astype(f32)
            ok = ln > 0
            return np.where(ok, a * r, a).astype(f32), np.where(ok, b * r, b).astype(f32), np.where(ok, c * r, c).astype(f32)
        nx, ny, nz = normalize(nx, ny, nz)
        lx, ly, lz = normalize((f32(5) - sx).astype(f32), (f32(5) - sy).astype(f32), (f32(10) - sz).astype(f32))
        dv = I._max_ieee((((nx * lx).astype(f32) + (ny * ly).astype(f32)).astype(f32) + (nz * lz).astype(f32)).astype(f32), np.zeros(k.shape, f32))
        bgm = np.where(depth > f32(farp), f32(1), f32(0)).astype(f32)
        fgm = np.where(bgm == 0, f32(1), f32(0)).astype(f32)
        rgb = [(f32(0) + ((((dv * dd).astype(f32) + f32(0.1)).astype(f32) * fgm).astype(f32) + (bgm * f32(bg)).astype(f32))).astype(f32)
               for dd, bg in ((d0, 0.5), (d1, 0.75), (d2, 1.0))]
    return depth.reshape(height, width), np.stack(rgb, -1).reshape(height, width, 3)


# ---- the interval bound (block culling) -----------------------------------------------------------------------------------------
def pyramid(data):
    """levels 1..top of the min/max pyramid of one channel: list of (lo, hi) arrays, NaN where a cell holds a non-finite value"""
    data = np.asarray(data, f32)
    bad = ~np.isfinite(data)
    lo = np.where(bad, f32(np.nan), data)
    hi = lo.copy()
    levels = [None]
    top = max(int(np.ceil(np.log2(n))) if n > 1 else 0 for n in data.shape)
    for _ in range(top):
        shp = [(n + 1) // 2 for n in lo.shape]
        pad = [(0, 2 * s - n) for s, n in zip(shp, lo.shape)]
        lp = np.pad(lo, pad, constant_values=np.inf).reshape(shp[0], 2, shp[1], 2, shp[2], 2)
        hp = np.pad(hi, pad, constant_values=-np.inf).reshape(shp[0], 2, shp[1], 2, shp[2], 2)
        # (nanmin would drop the poison: a NaN anywhere keeps the cell NaN)
        lo = np.where(np.isnan(lp).any(axis=(1, 3, 5)), f32(np.nan), lp.min(axis=(1, 3, 5))).astype(f32)
        hi = np.where(np.isnan(hp).any(axis=(1, 3, 5)), f32(np.nan), hp.max(axis=(1, 3, 5))).astype(f32)
        levels.append((lo, hi))
    return levels


def box_bound(data, levels, x0, x1, y0, y1, z0, z1):
    """(lo, hi) of the index box as the kernel reads it: NaN = unknown"""
    L = 0
    while (x1 >> L) - (x0 >> L) > 1 or (y1 >> L) - (y0 >> L) > 1 or (z1 >> L) - (z0 >> L) > 1:
        L += 1
    lo, hi = np.inf, -np.inf
    for k in range(8):
        cx, cy, cz = ((x1 if k & 1 else x0) >> L, (y1 if k & 2 else y0) >> L, (z1 if k & 4 else z0) >> L)
        if L == 0:
            v = float(data[cx, cy, cz])
            if not np.isfinite(v):
                return np.nan, np.nan
            a = b = v
        else:
            a, b = float(levels[L][0][cx, cy, cz]), float(levels[L][1][cx, cy, cz])
        if np.isnan(a) or np.isnan(b):
            return np.nan, np.nan
        lo, hi = min(lo, a), max(hi, b)
    return lo, hi


def interval(vol, ch, op, X, Y, Z, levels=None):
    """the interval form of a volume read over the box X x Y x Z ((lo, hi) pairs of floats)"""
    data = _channel(vol, ch)
    levels = levels if levels is not None else pyramid(data)
    n = data.shape
    if any(np.isnan(c[0]) or np.isnan(c[1]) for c in (X, Y, Z)):
        return np.nan, np.nan
    d = vol_d(vol)
    mn = np.asarray(vol[2], f32)
    box = []
    for a, c in enumerate((X, Y, Z)):
        if op == NEAREST:
            q = quot(np.array([c[0], c[1]], f32), mn[a], d[a])
            i = near_idx(q, n[a])
            box += [int(i[0]), int(i[1])]
        else:
            m = f32(mn[a] + f32(f32(0.5) * d[a]))
            u = lin_u(np.array([c[0], c[1]], f32), m, d[a], n[a])
            i = lin_i0(u, n[a])
            box += [int(i[0]), int(i[1]) + (1 if n[a] > 1 else 0)]
    return box_bound(data, levels, *box)
