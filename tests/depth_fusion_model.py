"""numpy model of sdfk_volume_integrate_depth / sdfk_depth_unproject (include/sdfkit_hip.h, "Depth images: fusion and unprojection";
sdfkit_amd/csrc/depth_fusion.h): every operation of the header in its order on float32 arrays (numpy's float32 + - * / and sqrt
are correctly rounded and never fused), so the library's results equal these bit for bit.  Vectorised over the voxels."""
import numpy as np

from tests import mesh_ray_model as RM

f32, i64 = np.float32, np.int64
CARVE_BEYOND = 1


def grid_constants(mn, mx, n):
    """(d, m): the f32 cell sizes (max - min) / n and first cell centres min + 0.5 d"""
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    d = np.array([f32((mx[a] - mn[a]) / f32(n[a])) for a in range(3)], f32)
    m = np.array([f32(mn[a] + f32(f32(0.5) * d[a])) for a in range(3)], f32)
    return d, m


def centres(mn, mx, n, z0=0, nz_local=None):
    """The f32 cell centres of the volume (or of the slab of planes [z0, z0 + nz_local)) as three (nx, ny, nz) arrays."""
    nx, ny, nzg = n
    nz = nzg - z0 if nz_local is None else nz_local
    d, m = grid_constants(mn, mx, n)
    ax = [(m[0] + np.arange(nx).astype(f32) * d[0]).astype(f32), (m[1] + np.arange(ny).astype(f32) * d[1]).astype(f32),
          (m[2] + (z0 + np.arange(nz)).astype(f32) * d[2]).astype(f32)]
    return [np.ascontiguousarray(a) for a in np.meshgrid(*ax, indexing="ij")]


def project(p, m, width, height):
    """Steps 1 and 2 -> (seen bool, pixel int64 (0 where not seen))"""
    m = np.asarray(m, f32).reshape(-1)
    with np.errstate(all="ignore"):
        c = {q: ((p[0] * m[q] + p[1] * m[4 + q]) + p[2] * m[8 + q]) + m[12 + q] for q in (0, 1, 3)}
        wm, hm = f32(width - 1), f32(height - 1)
        u = (c[0] / c[3] + f32(1)) * f32(wm * f32(0.5))
        v = (f32(1) - c[1] / c[3]) * f32(hm * f32(0.5))
        fu, fv = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        seen = (c[3] > 0) & (fu >= 0) & (fu <= wm) & (fv >= 0) & (fv <= hm)
        pix = np.where(seen, fv, 0).astype(i64) * width + np.where(seen, fu, 0).astype(i64)
    assert all(a.dtype == f32 for a in (u, v, fu, fv))
    return seen, pix


def integrate(D, W, mn, mx, depth, cam, vp, truncation, depth_min, depth_max, weight=1.0, max_weight=np.inf, flags=0, z0=0, nz_global=None):
    """One frame -> (D', W', stats[4]).  D, W: (nx, ny, nz) float32, the planes [z0, z0 + nz) of a volume of nz_global planes."""
    D, W = np.asarray(D, f32), np.asarray(W, f32)
    depth = np.asarray(depth, f32)
    height, width = depth.shape
    nx, ny, nz = D.shape
    nzg = nz if nz_global is None else nz_global
    trunc, dmin, dmax, wt, maxw = f32(truncation), f32(depth_min), f32(depth_max), f32(weight), f32(max_weight)
    cam = np.asarray(cam, f32).reshape(-1)
    p = centres(mn, mx, (nx, ny, nzg), z0, nz)
    seen, pix = project(p, vp, width, height)
    with np.errstate(all="ignore"):
        d = depth.reshape(-1)[pix]
        dx, dy, dz = p[0] - cam[0], p[1] - cam[1], p[2] - cam[2]
        r = np.sqrt((dx * dx + dy * dy) + dz * dz)
        s = d - r
        valid = (d >= dmin) & (d <= dmax)
        surface = seen & valid & ~(s < -trunc)
        within = surface & (s <= trunc)
        carved = seen & ~valid & bool(flags & CARVE_BEYOND) & (d > dmax) & (r <= dmax)
        upd = surface | carved
        t = np.where(within, s, trunc).astype(f32)
        old = W > 0
        tot = W + wt
        avg = (W * D + wt * t) / tot
        D1 = np.where(upd, np.where(old, avg, t), D).astype(f32)
        W1 = np.where(upd, np.where(old, np.where(tot <= maxw, tot, maxw), np.where(wt <= maxw, wt, maxw)), W).astype(f32)
        assert r.dtype == f32 and s.dtype == f32 and avg.dtype == f32
        npix = int(((depth >= dmin) & (depth <= dmax)).sum())
    # (np.where moves float32 values as they are: the bits of a voxel that is not updated stay)
    return D1, W1, [int(upd.sum()), int(within.sum()), int((upd & ~old).sum()), npix]


def unproject(depth, cam, vpi, depth_min, depth_max, rgb=None):
    """-> (points (n, 3) f32, colors (n, 3) f32 or None, pixel (n,) int32)"""
    depth = np.asarray(depth, f32)
    height, width = depth.shape
    cam = np.asarray(cam, f32).reshape(-1)
    d = depth.reshape(-1)
    with np.errstate(all="ignore"):
        valid = np.flatnonzero((d >= f32(depth_min)) & (d <= f32(depth_max)))
        R = RM.camera_rays(width, height, cam, vpi)[valid]
        pts = np.stack([(cam[a] + (R[:, a] * d[valid]).astype(f32)).astype(f32) for a in range(3)], -1).reshape(-1, 3)
    cols = None if rgb is None else np.asarray(rgb, f32).reshape(-1, 3)[valid]
    return pts, cols, valid.astype(np.int32)


# ---- accuracy: the zero set of a fused volume against the scene ----------------------------------------------------------------
def sphere_depth(width, height, cam, vpi, spheres):
    """The analytic depth along the camera rays of the library's own camera arithmetic to the nearest of `spheres`
    ((centre, radius), ...), float64 geometry rounded once to float32; +inf where a ray misses."""
    R = RM.camera_rays(width, height, cam, vpi).astype(np.float64)
    o = np.asarray(cam, np.float64)
    best = np.full(len(R), np.inf)
    for c, rad in spheres:
        oc = o - np.asarray(c, np.float64)
        b = (R[:, 0] * oc[0] + R[:, 1] * oc[1]) + R[:, 2] * oc[2]   # (no BLAS: one order of operations everywhere)
        disc = b * b - (((oc[0] * oc[0] + oc[1] * oc[1]) + oc[2] * oc[2]) - rad * rad)
        with np.errstate(all="ignore"):
            t = -b - np.sqrt(disc)
        t = np.where((disc >= 0) & (t > 0), t, np.inf)
        best = np.minimum(best, t)
    return best.astype(f32).reshape(height, width)


def zero_crossings(D, mn, mx, sdf):
    """|sdf| at the linear zero crossings of D on the grid's edges, in voxels (the cells are cubes): (max, mean, count)."""
    nx, ny, nz = D.shape
    p = [a.astype(np.float64) for a in centres(mn, mx, D.shape)]
    h = float(grid_constants(mn, mx, D.shape)[0][0])
    D = D.astype(np.float64)
    errs = []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        a, b = D[lo], D[hi]
        cross = (a > 0) != (b > 0)
        f = a[cross] / (a[cross] - b[cross])
        q = [c[lo][cross] + f * (c[hi][cross] - c[lo][cross]) for c in p]
        errs.append(np.abs(sdf(*q)) / h)
    e = np.concatenate(errs)
    return float(e.max()), float(e.mean()), int(len(e))


def wrong_signs(D, mn, mx, sdf):
    """Voxels farther than one voxel from the surface whose sign is not the scene's."""
    p = [a.astype(np.float64) for a in centres(mn, mx, D.shape)]
    h = float(grid_constants(mn, mx, D.shape)[0][0])
    true = sdf(*p)
    return int((((D > 0) != (true > 0)) & (np.abs(true) > h)).sum())


# ---- the accuracy set-ups: closed scans of analytic scenes through the model ------------------------------------------------------
VIEWS14 = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] + [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
SCENES = {"sphere": (((0.0, 0.0, 0.0), 1.0),), "two_spheres": (((-0.6, 0.0, 0.0), 0.5), ((0.65, 0.0, 0.0), 0.4))}


def view(k, n=14):
    """Camera k of the scan: on the ray of VIEWS14[k] at distance 4 .. 4.3 from the origin, looking at it."""
    v = np.asarray(VIEWS14[k], np.float64)
    pos = v / np.sqrt(v @ v) * (4.0 + 0.3 * k / (n - 1))
    up = (0.0, 0.0, 1.0) if VIEWS14[k][0] == 0 and VIEWS14[k][2] == 0 else (0.0, 1.0, 0.0)
    return (tuple(float(x) for x in pos), (0.0, 0.0, 0.0), up)


def scene_sdf(scene):
    def sdf(x, y, z):
        return np.minimum.reduce([np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r for c, r in SCENES[scene]])
    return sdf


def scan(scene, n, pixels, views, carve, camera):
    """The model's fused volume of `scene` in the box -+1.5 at n^3 from the given views of pixels^2 analytic depth frames,
    truncation three voxels, weight 1; filled with -truncation (carve) or +truncation (open).  camera: (width, height, view) ->
    (position, view_projection, inverse, near, far), the library's host arithmetic."""
    mn, mx = (-1.5,) * 3, (1.5,) * 3
    trunc = f32(3.0 * 3.0 / n)
    D, W = np.full((n, n, n), -trunc if carve else trunc, f32), np.zeros((n, n, n), f32)
    for k in views:
        pos, vp, vpi, near, far = camera(pixels, pixels, view(k))
        depth = sphere_depth(pixels, pixels, pos, vpi, SCENES[scene])
        D, W, _ = integrate(D, W, mn, mx, depth, pos, vp, trunc, near, far, 1.0, np.inf, CARVE_BEYOND if carve else 0)
    return D, mn, mx


def accuracy(scene, n, pixels, views, carve, camera):
    D, mn, mx = scan(scene, n, pixels, views, carve, camera)
    sdf = scene_sdf(scene)
    emax, emean, count = zero_crossings(D, mn, mx, sdf)
    return {"wrong_signs_beyond_one_voxel": wrong_signs(D, mn, mx, sdf), "crossing_error_max_voxels": round(emax, 6),
            "crossing_error_mean_voxels": round(emean, 6), "crossings": count}
