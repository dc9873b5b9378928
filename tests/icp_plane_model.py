"""A numpy restatement of the point-to-plane metric of IterativeClosestPoint (sdfk_icp_register_plane: include/sdfkit_hip.h,
"IterativeClosestPoint.RegisterPoints, point to plane"), the yardstick of csrc/icp_solve.h's plane part and of the kernels of
csrc/lib_points.hip.  Not a test module.

The search (nearest), the reduction order (reduce_fixed), the distMax rule and the f32 Matrix4x4 arithmetic are those of
tests/points_model.py; everything else is written here, one numpy float64 operation per written operation:

- plane_row_exact(): one kept point's row J = (d x n, n), d = p - pmean, and residual r = (p - q) . n;
- jacobi6_exact(), pinv_solve6_exact(): cyclic Jacobi on the symmetric 6x6 A and x = sum_k v_k (v_k . (-b)) / lambda_k over the
  eigenpairs with lambda_k > TAU lambda_max;
- cayley_step_exact(), solve_step_plane_exact(): the rotation of w = x[0..2] / 2, the translation, the f32 step, convergence, total;
- plane_step_exact(), register_plane_exact(): one iteration and the whole registration, bit for bit what the library returns.
"""
import numpy as np

from sdfkit_amd.raymarch import Matrix4x4
from tests.points_model import converged, dist_max_exact, nearest, reduce_fixed, transform_points

f32, f64 = np.float32, np.float64
SWEEPS6 = 8                  # kSweeps6 of icp_solve.h
TAU = f64(1e-12)             # kPlaneTau of icp_solve.h
PAIRS6 = [(p, q) for p in range(5) for q in range(p + 1, 6)]
UPPER6 = [(a, b) for a in range(6) for b in range(a, 6)]      # the order of the 21 products J_a J_b


def plane_row_exact(p, q, n, pmean):
    """-> (J (6,), r): p, q, n float32 (widened first), pmean float64."""
    p, q, n = [np.asarray(v, f32).astype(f64) for v in (p, q, n)]
    pmean = np.asarray(pmean, f64)
    with np.errstate(all="ignore"):
        d = [p[a] - pmean[a] for a in range(3)]
        c = [d[1] * n[2] - d[2] * n[1], d[2] * n[0] - d[0] * n[2], d[0] * n[1] - d[1] * n[0]]
        r = ((p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1]) + (p[2] - q[2]) * n[2]
    return np.array(c + [n[0], n[1], n[2]], f64), f64(r)


def unpack21(A21):
    A = np.zeros((6, 6), f64)
    for k, (a, b) in enumerate(UPPER6):
        A[a, b] = A[b, a] = A21[k]
    return A


def jacobi6_exact(A21, sweeps=SWEEPS6, info=None):
    """jacobi6 of icp_solve.h -> (lambda (6,), V (6, 6), the eigenvectors its columns).  `info` receives rotations and last_change:
    the last sweep (1-based) that changed lambda or V."""
    A0 = unpack21(np.asarray(A21, f64))
    a = [[A0[i, j] for j in range(6)] for i in range(6)]
    one, zero = f64(1.0), f64(0.0)
    v = [[one if i == j else zero for j in range(6)] for i in range(6)]
    rotations, last_change = 0, 0
    with np.errstate(all="ignore"):
        for sweep in range(sweeps):
            before = ([a[i][i] for i in range(6)], [row[:] for row in v]) if info is not None else None
            for p, q in PAIRS6:
                apq = a[p][q]
                if apq == 0.0:
                    continue
                rotations += 1
                theta = (a[q][q] - a[p][p]) / (f64(2.0) * apq)
                at = -theta if theta < 0.0 else theta
                t = one / (at + np.sqrt(theta * theta + one))
                if theta < 0.0:
                    t = -t
                c = one / np.sqrt(t * t + one)
                s = t * c
                a[p][p] = a[p][p] - t * apq
                a[q][q] = a[q][q] + t * apq
                a[p][q] = a[q][p] = zero
                for r in range(6):
                    if r == p or r == q:
                        continue
                    arp, arq = a[r][p], a[r][q]
                    a[r][p] = a[p][r] = c * arp - s * arq
                    a[r][q] = a[q][r] = s * arp + c * arq
                for k in range(6):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - s * vkq
                    v[k][q] = s * vkp + c * vkq
            if info is not None:
                now = np.array([a[i][i] for i in range(6)] + sum(v, []), f64)
                was = np.array(before[0] + sum(before[1], []), f64)
                if not np.array_equal(now.view(np.uint64), was.view(np.uint64)):
                    last_change = sweep + 1
    if info is not None:
        info.update(rotations=rotations, last_change=last_change)
    return np.array([a[i][i] for i in range(6)], f64), np.array(v, f64)


def pinv_solve6_exact(A21, b, info=None, sweeps=SWEEPS6):
    """pinv_solve6 of icp_solve.h -> (x (6,), retained, lambda (6,))."""
    lam, V = jacobi6_exact(A21, sweeps, info)
    b = np.asarray(b, f64)
    x = [f64(0.0)] * 6
    retained = 0
    lmax = lam[0]
    for k in range(1, 6):
        if lam[k] > lmax:
            lmax = lam[k]
    with np.errstate(all="ignore"):
        if lmax > 0.0 and lmax < np.inf:
            cut = TAU * lmax
            for k in range(6):
                if not lam[k] > cut:
                    continue
                retained += 1
                dot = f64(0.0)
                for a in range(6):
                    dot = dot + V[a, k] * (-b[a])
                coef = dot / lam[k]
                for a in range(6):
                    x[a] = x[a] + V[a, k] * coef
    return np.array(x, f64), retained, lam


def cayley_step_exact(x, pmean):
    """cayley_step of icp_solve.h -> (R (3, 3), T (3,)), float64."""
    x, pm = np.asarray(x, f64), np.asarray(pmean, f64)
    one, two = f64(1.0), f64(2.0)
    with np.errstate(all="ignore"):
        w = [x[a] / two for a in range(3)]
        ww = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        om, den = one - ww, one + ww
        R = np.empty((3, 3), f64)
        for a in range(3):
            R[a, a] = (om + two * (w[a] * w[a])) / den
        R[0, 1] = (two * (w[0] * w[1]) - two * w[2]) / den
        R[1, 0] = (two * (w[0] * w[1]) + two * w[2]) / den
        R[0, 2] = (two * (w[0] * w[2]) + two * w[1]) / den
        R[2, 0] = (two * (w[0] * w[2]) - two * w[1]) / den
        R[1, 2] = (two * (w[1] * w[2]) - two * w[0]) / den
        R[2, 1] = (two * (w[1] * w[2]) + two * w[0]) / den
        T = np.array([(pm[a] + x[3 + a]) - ((R[a, 0] * pm[0] + R[a, 1] * pm[1]) + R[a, 2] * pm[2]) for a in range(3)], f64)
    return R, T


def solve_step_plane_exact(A21, b, pmean, total_prev, max_t=f32(1e-4), max_r=f32(1e-5), info=None, sweeps=SWEEPS6):
    """solve_step_plane of icp_solve.h -> (x, retained, lambda, R, T, step, total, converged)."""
    x, retained, lam = pinv_solve6_exact(A21, b, info, sweeps)
    R, T = cayley_step_exact(x, pmean)
    with np.errstate(all="ignore"):
        step = np.eye(4, dtype=f32)
        step[:3, :3] = R.T.astype(f32)
        step[3, :3] = T.astype(f32)
        conv = converged(step, f32(max_t), f32(max_r))[0]
        total = Matrix4x4.Multiply(np.asarray(total_prev, f32).reshape(4, 4), step)
    return x, retained, lam, R, T, step, total, conv


def plane_step_exact(static, normals, points, total_prev, good=f32(0.01), max_t=f32(1e-4), max_r=f32(1e-5)):
    """One iteration as the device runs it: -> (step, total, converged, details).  `points` is not modified."""
    static, normals = np.asarray(static, f32).reshape(-1, 3), np.asarray(normals, f32).reshape(-1, 3)
    idx, dist, cor = nearest(static, points)
    n = len(dist)
    with np.errstate(all="ignore"):
        d = dist.astype(f64)
        mean = reduce_fixed(d) / f64(n)
        dm = d - mean
        sqsum = reduce_fixed(dm * dm)
        dmax, bracket, m, sd = dist_max_exact(mean, sqsum, n, good)
        nrm = normals[np.maximum(idx, 0)]
        keep = (dist <= dmax) & (idx >= 0) & ~((nrm[:, 0] == 0) & (nrm[:, 1] == 0) & (nrm[:, 2] == 0))
        p, q, nn = points.astype(f64), cor.astype(f64), nrm.astype(f64)
        sums = reduce_fixed(np.where(keep[:, None], np.concatenate([np.ones((n, 1)), p], axis=1), 0.0))
        pmean = sums[1:4] / sums[0]
        dd = p - pmean
        c = np.stack([dd[:, 1] * nn[:, 2] - dd[:, 2] * nn[:, 1], dd[:, 2] * nn[:, 0] - dd[:, 0] * nn[:, 2],
                      dd[:, 0] * nn[:, 1] - dd[:, 1] * nn[:, 0]], axis=1)
        J = np.concatenate([c, nn], axis=1)
        r = ((p[:, 0] - q[:, 0]) * nn[:, 0] + (p[:, 1] - q[:, 1]) * nn[:, 1]) + (p[:, 2] - q[:, 2]) * nn[:, 2]
        cols = np.stack([J[:, a] * J[:, b] for a, b in UPPER6] + [J[:, a] * r for a in range(6)] + [r * r], axis=1)
        red = reduce_fixed(np.where(keep[:, None], cols, 0.0))
    info = {}
    A21, b, rsq = red[:21], red[21:27], red[27]
    x, retained, lam, R, T, step, total, conv = solve_step_plane_exact(A21, b, pmean, total_prev, max_t, max_r, info)
    info.update(dist_max=dmax, bracket=bracket, kept=int(sums[0]) if np.isfinite(sums[0]) else 0, pmean=pmean, A=unpack21(A21), b=b, rsq=rsq, x=x,
                retained=retained, lam=lam, R=R, T=T, keep=keep)
    return step, total, conv, info


def register_plane_exact(static, normals, points, max_iterations=100, good=f32(0.01), max_t=f32(1e-4), max_r=f32(1e-5)):
    """sdfk_icp_register_plane bit for bit: moves `points` ((n, 3) float32) in place; -> (total, iterations, [total after each
    iteration], [details of each iteration, "points": the moved points after it, "stats": the int64[4] after it])."""
    total = np.eye(4, dtype=f32)
    totals, infos = [], []
    done = False
    it = 0
    while not done and it < max_iterations:
        step, total, done, info = plane_step_exact(static, normals, points, total, good, max_t, max_r)
        with np.errstate(all="ignore"):
            points[:] = transform_points(points, step)
        totals.append(total)
        info["points"] = points.copy()
        info["stats"] = np.array([info["kept"], int(np.array(info["rsq"], f64).view(np.int64)), int(done), info["retained"]], np.int64)
        infos.append(info)
        it += 1
    return total, it, totals, infos


# ---- the clouds of the tests ----
def height(x, y):
    return 0.25 * np.sin(3 * x) * np.cos(2 * y) + 0.1 * x * y


def height_field_static(m=48):
    """the m x m grid over [-1, 1]^2 of z = 0.25 sin(3x) cos(2y) + 0.1 x y with its analytic unit normals -> (points, normals) float32"""
    g = np.linspace(-1, 1, m)
    X, Y = np.meshgrid(g, g, indexing="ij")
    S = np.stack([X, Y, height(X, Y)], -1).reshape(-1, 3)
    fx = 0.75 * np.cos(3 * X) * np.cos(2 * Y) + 0.1 * Y
    fy = -0.5 * np.sin(3 * X) * np.sin(2 * Y) + 0.1 * X
    Nn = np.stack([-fx, -fy, np.ones_like(fx)], -1).reshape(-1, 3)
    Nn /= np.linalg.norm(Nn, axis=1, keepdims=True)
    return S.astype(f32), Nn.astype(f32)


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def height_field_dynamic(n, seed=5):
    """n off-grid surface points (uniform in [-0.8, 0.8]^2), and the same rotated by the vector (0.03, -0.02, 0.04) and moved by
    (0.03, -0.02, 0.015) -> (true positions float64, moved points float32)"""
    u = np.random.default_rng(seed).uniform(-0.8, 0.8, (n, 2))
    D0 = np.stack([u[:, 0], u[:, 1], height(u[:, 0], u[:, 1])], -1)
    D = D0 @ _rodrigues(np.array([0.03, -0.02, 0.04])).T + np.array([0.03, -0.02, 0.015])
    return D0, D.astype(f32)


def plane_case():
    """a 16 x 16 grid on z = 0 with normals (0, 0, 1); the same points lifted by 0.5 and tilted about x by 1/16"""
    g = (np.arange(16, dtype=f32) - f32(7.5)) * f32(0.125)
    S = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    S = np.concatenate([S, np.zeros((len(S), 1), f32)], axis=1).astype(f32)
    Nn = np.tile(np.array([0, 0, 1], f32), (len(S), 1))
    D = S.copy()
    D[:, 2] = f32(0.5) + S[:, 1] * f32(0.0625)
    return S, Nn, D


def rms(a, b):
    return float(np.sqrt(((np.asarray(a, f64) - np.asarray(b, f64)) ** 2).sum(axis=1).mean()))
