"""The numpy model of sdfk_trimesh_raycast / sdfk_trimesh_render (include/sdfkit_hip.h, "Triangle meshes: ray casting"): brute force
over ALL triangles in float64 with the header's operation order -- the watertight test of Woop, Benthin and Wald, the (t, index)
minimum, the any-hit rule -- the camera rays of the ray marcher (mirrored from tests/voxel_sdf_model.py raymarch, which mirrors the
kernel) and the Lambert shading.  No grid, no walk: what the library's walk must reproduce bit for bit."""
from collections import namedtuple

import numpy as np

f32, f64, i32 = np.float32, np.float64, np.int32
ANY_HIT = 1

Hits = namedtuple("Hits", "triangle distance weights")
CHUNK_ELEMS = 1 << 19   # rays x triangles per block: some forty float64 temporaries of 4 MiB each


def _setup(D):
    """kz (greatest |d|, ties to the lowest axis), kx, ky (swapped when d[kz] < 0) per ray"""
    ad = np.abs(D)
    kz = np.zeros(len(D), np.int64)
    am = ad[:, 0].copy()
    for a in (1, 2):
        m = ad[:, a] > am
        kz[m] = a
        am[m] = ad[m, a]
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    neg = D[np.arange(len(D)), kz] < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    return kx, ky, kz


def bad_rays(O, D):
    O, D = np.asarray(O, f32).reshape(-1, 3), np.asarray(D, f32).reshape(-1, 3)
    return ~(np.all(np.isfinite(O), 1) & np.all(np.isfinite(D), 1)) | np.all(D == 0, 1)


def cast(V, T, O, D, tmin=0.0, tmax=np.inf, flags=0):
    """-> Hits(triangle (n,) int32, distance (n,) f32, weights (n, 3) f32); with ANY_HIT triangle is 0 / -1 and the rest None"""
    V = np.asarray(V, f32).reshape(-1, 3).astype(f64)
    T = np.asarray(T, i32).reshape(-1, 3)
    O32, D32 = np.asarray(O, f32).reshape(-1, 3), np.asarray(D, f32).reshape(-1, 3)
    n, nt = len(O32), len(T)
    tmin, tmax = f64(f32(tmin)), f64(f32(tmax))
    tri = np.full(n, -1, i32)
    dist = np.full(n, np.inf, f32)
    wts = np.full((n, 3), np.nan, f32)
    good = np.flatnonzero(~bad_rays(O32, D32))
    Og, Dg = O32[good].astype(f64), D32[good].astype(f64)
    kx, ky, kz = _setup(Dg)
    a, b, c = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    step = max(1, CHUNK_ELEMS // max(nt, 1))
    with np.errstate(all="ignore"):
        for gx, gy, gz in ((1, 2, 0), (2, 1, 0), (2, 0, 1), (0, 2, 1), (0, 1, 2), (1, 0, 2)):
            grp = np.flatnonzero((kx == gx) & (ky == gy) & (kz == gz))
            for s in range(0, len(grp), step):
                r = grp[s:s + step]
                o, d = Og[r], Dg[r]
                Sx, Sy, Sz = (d[:, gx] / d[:, gz])[:, None], (d[:, gy] / d[:, gz])[:, None], (1.0 / d[:, gz])[:, None]
                P = []
                for p in (a, b, c):
                    pz = p[None, :, gz] - o[:, None, gz]
                    P.append((p[None, :, gx] - o[:, None, gx] - Sx * pz, p[None, :, gy] - o[:, None, gy] - Sy * pz, pz))
                (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = P
                U, Vv, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
                miss = ((U < 0) | (Vv < 0) | (W < 0)) & ((U > 0) | (Vv > 0) | (W > 0))
                det = (U + Vv) + W
                Tt = (U * (Sz * Az) + Vv * (Sz * Bz)) + W * (Sz * Cz)
                t = Tt / det
                hit = ~miss & (det != 0) & (t >= tmin) & (t <= tmax) & np.isfinite(t)
                any_ = hit.any(1)
                if flags & ANY_HIT:
                    tri[good[r]] = np.where(any_, 0, -1)
                    continue
                best = np.argmin(np.where(hit, t, np.inf), 1)   # (the first of equal minima: the lowest index)
                rows = np.arange(len(r))
                bt, bd = t[rows, best], det[rows, best]
                out = good[r[any_]]
                tri[out] = best[any_]
                dist[out] = bt[any_].astype(f32)
                for q, X in enumerate((U, Vv, W)):
                    wts[out, q] = (X[rows, best] / bd)[any_].astype(f32)
    if flags & ANY_HIT:
        return Hits(tri, None, None)
    return Hits(tri, dist, wts)


def camera_rays(width, height, cam, m):
    """the unit rays of sdfk_raymarch's kernel, row-major (k = j width + i): (width * height, 3) float32"""
    with np.errstate(all="ignore"):
        k = np.arange(width * height)
        j, i = k // width, k % width
        y = (f32(1) - (f32(2) * j.astype(f32)).astype(f32) / f32(height - 1)).astype(f32)
        x = (f32(-1) + (f32(2) * i.astype(f32)).astype(f32) / f32(width - 1)).astype(f32)
        m = np.asarray(m, f32).reshape(-1)
        cam = np.asarray(cam, f32).reshape(-1)
        v4 = [((((x * m[q]).astype(f32) + (y * m[4 + q]).astype(f32)).astype(f32) + (f32(0) * m[8 + q]).astype(f32)).astype(f32)
               + (f32(1) * m[12 + q]).astype(f32)).astype(f32) for q in range(4)]
        dx, dy, dz = (((v4[a] / v4[3]).astype(f32) - cam[a]).astype(f32) for a in range(3))
        dl = np.sqrt((((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)).astype(f32)).astype(f32)
        return np.stack([(dx / dl).astype(f32), (dy / dl).astype(f32), (dz / dl).astype(f32)], -1)


def _normalize_inplace(a, b, c):
    ln = np.sqrt((((a * a).astype(f32) + (b * b).astype(f32)).astype(f32) + (c * c).astype(f32)).astype(f32)).astype(f32)
    r = (f32(1) / ln).astype(f32)
    ok = ln > 0
    return np.where(ok, a * r, a).astype(f32), np.where(ok, b * r, b).astype(f32), np.where(ok, c * r, c).astype(f32)


def render(V, T, colors, width, height, cam, m, nearp, farp):
    """-> (depth [h, w] f32, rgb [h, w, 3] f32, triangle [h, w] int32)"""
    V32 = np.asarray(V, f32).reshape(-1, 3)
    T = np.asarray(T, i32).reshape(-1, 3)
    cam = np.asarray(cam, f32).reshape(-1)
    R = camera_rays(width, height, cam, m)
    n = len(R)
    H = cast(V32, T, np.broadcast_to(cam, (n, 3)), R, nearp, farp)
    hit = H.triangle >= 0
    rgb = np.empty((n, 3), f32)
    rgb[:] = np.array([0.5, 0.75, 1.0], f32)
    with np.errstate(all="ignore"):
        if hit.any():
            t = T[H.triangle[hit]]
            r, dist, w = R[hit], H.distance[hit], H.weights[hit]
            s = [(cam[a] + (r[:, a] * dist).astype(f32)).astype(f32) for a in range(3)]
            a, b, c = (V32[t[:, q]].astype(f64) for q in range(3))
            e1, e2 = b - a, c - a
            n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            ln = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
            ok = ln > 0
            nx, ny, nz = (np.where(ok, q / ln, 0.0).astype(f32) for q in (n0, n1, n2))
            along = (((nx * r[:, 0]).astype(f32) + (ny * r[:, 1]).astype(f32)).astype(f32) + (nz * r[:, 2]).astype(f32)).astype(f32) > 0
            nx, ny, nz = (np.where(along, -q, q).astype(f32) for q in (nx, ny, nz))
            lx, ly, lz = _normalize_inplace((f32(5) - s[0]).astype(f32), (f32(5) - s[1]).astype(f32), (f32(10) - s[2]).astype(f32))
            nl = (((nx * lx).astype(f32) + (ny * ly).astype(f32)).astype(f32) + (nz * lz).astype(f32)).astype(f32)
            dv = np.where(np.isnan(nl), nl, np.where(nl > 0, nl, f32(0))).astype(f32)
            for k in range(3):
                if colors is None:
                    col = np.ones(len(t), f32)
                else:
                    C = np.asarray(colors, f32).reshape(-1, 3)
                    ca, cb, cc = C[t[:, 0], k], C[t[:, 1], k], C[t[:, 2], k]
                    col = (((ca * w[:, 0]).astype(f32) + (cb * w[:, 1]).astype(f32)).astype(f32) + (cc * w[:, 2]).astype(f32)).astype(f32)
                rgb[hit, k] = ((dv * col).astype(f32) + f32(0.1)).astype(f32)
    return H.distance.reshape(height, width), rgb.reshape(height, width, 3), H.triangle.reshape(height, width)
