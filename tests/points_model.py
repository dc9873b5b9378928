"""A numpy restatement of SdfKit's KdTree.Search and IterativeClosestPoint.RegisterPoints, the yardstick of the GPU
search and registration (sdfkit_amd.points, csrc/lib_points.hip).  Not a test module.

- nearest(): brute force over every static point with the contract's formula: d2 = (dx*dx + dy*dy) + dz*dz in float32
  (numpy float32 arithmetic has no FMA), the least d2 wins, ties to the lowest index, distance = sqrtf(d2) correctly
  rounded; a point counts only if its distance is < FLT_MAX; none: index -1, distance FLT_MAX, nearest = first point.
- register(): the reference's ICP iteration (IterativeClosestPoint.cs:53-196) with the library's stated precision: f64
  reductions and np.linalg.svd, then R, pmean, qmean rounded to float32 and the reference's float32 Matrix4x4 steps
  (sdfkit_amd.raymarch.Matrix4x4: Invert, Multiply, CreateTranslation, Transform).
- reduce_fixed(), kabsch_r_exact(), icp_step_exact(), register_exact(): the same iteration bit for bit -- the device's reduction
  order and the arithmetic of csrc/icp_solve.h, one numpy operation per written operation (include/sdfkit_hip.h states both).
  register() above stays as the independent (LAPACK, pairwise sums) check at 1e-6.
- NetRandom: System.Random(seed), the BCL's seeded subtractive generator, restated from its published algorithm (Knuth's
  subtractive method) for the reference tests' Random(0) inputs.  It cannot be checked against .NET here: no assertion may
  depend on its exact values.
"""
import numpy as np

from sdfkit_amd.raymarch import Matrix4x4

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def nearest(static, queries, chunk_elems=1 << 24):
    """-> (index int32, distance float32, nearest (m, 3) float32) of every query."""
    P = np.ascontiguousarray(np.asarray(static, f32).reshape(-1, 3))
    Q = np.ascontiguousarray(np.asarray(queries, f32).reshape(-1, 3))
    m = len(Q)
    idx = np.full(m, -1, np.int32)
    d2min = np.full(m, np.inf, f32)
    step = max(1, chunk_elems // max(1, len(P)))
    with np.errstate(all="ignore"):
        for a in range(0, m, step):
            q = Q[a:a + step]
            dx = q[:, None, 0] - P[None, :, 0]
            dy = q[:, None, 1] - P[None, :, 1]
            dz = q[:, None, 2] - P[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            d2[~(d2 < np.inf)] = np.inf         # NaN / inf: does not count
            j = np.argmin(d2, axis=1)           # (first occurrence: the lowest index on ties)
            best = d2[np.arange(len(q)), j]
            ok = best < np.inf
            idx[a:a + step] = np.where(ok, j, -1)
            d2min[a:a + step] = best
    dist = np.where(idx >= 0, np.sqrt(d2min.astype(np.float64)).astype(f32), FLT_MAX).astype(f32)
    near = np.where((idx >= 0)[:, None], P[np.maximum(idx, 0)], P[0][None, :]).astype(f32)
    return idx, dist, near


def transform_points(points, m):
    """Vector3.Transform of every row (float32, ((x M11 + y M21) + z M31) + M41 ...)."""
    m = np.asarray(m, f32)
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    return np.stack([((x * m[0, j] + y * m[1, j]) + z * m[2, j]) + m[3, j] for j in range(3)], axis=1).astype(f32)


def kabsch_r(C):
    """R = V diag(1, 1, sign det(V U^T)) U^T of C = U S V^T (f64)."""
    U, _, Vt = np.linalg.svd(C)
    V = Vt.T
    d = np.sign(np.linalg.det(V @ U.T))
    return V @ np.diag([1.0, 1.0, d]) @ U.T


def icp_step(static, points, good=f32(0.01), textbook=False):
    """One GetIterTransform: -> (step matrix, details).  `points` is not modified.  textbook=True: the translation that
    carries the filtered mean of p onto that of q (what the reference does NOT do), for comparison."""
    _, dist, cor = nearest(static, points)
    d = dist.astype(np.float64)
    n = len(d)
    mean = d.sum() / n
    var = ((d - mean) ** 2).sum() / n          # two passes, as IterativeClosestPoint.cs:95-100
    m, sd = f32(mean), f32(np.sqrt(var))
    if m < good:
        dmax = m + f32(3.0) * sd
    elif m < f32(3.0) * good:
        dmax = m + f32(2.0) * sd
    elif m < f32(6.0) * good:
        dmax = m + sd
    else:
        dmax = (m + f32(0.5)) + sd
    keep = dist <= dmax
    p = points[keep].astype(np.float64)
    q = cor[keep].astype(np.float64)
    pmean, qmean = p.mean(axis=0), q.mean(axis=0)
    C = (p - pmean).T @ (q - qmean)
    R = kabsch_r(C)
    rm = np.eye(4, dtype=f32)
    rm[:3, :3] = R.astype(f32)
    _, inv_r = Matrix4x4.Invert(rm)
    pm, qm = pmean.astype(f32), qmean.astype(f32)
    if textbook:
        t = Matrix4x4.Transform(pm, rm) - qm   # the rotated p mean onto the q mean
    else:
        t = Matrix4x4.Transform(pm, inv_r) - qm
    xf = Matrix4x4.Multiply(rm, Matrix4x4.CreateTranslation(t))
    _, step = Matrix4x4.Invert(xf)
    return step, {"dist_max": dmax, "kept": int(keep.sum()), "pmean": pm, "qmean": qm, "R": R, "translation": t}


def converged(step, max_t=f32(1e-4), max_r=f32(1e-5)):
    drot = (abs(f32(1) - step[0, 0]) + abs(f32(1) - step[1, 1])) + abs(f32(1) - step[2, 2])
    dtrans = f32(np.sqrt(np.float64((step[3, 0] * step[3, 0] + step[3, 1] * step[3, 1]) + step[3, 2] * step[3, 2])))
    return bool(dtrans <= max_t and drot <= max_r), float(dtrans), float(drot)


def register(static, points, max_iterations=100, good=f32(0.01), max_t=f32(1e-4), max_r=f32(1e-5), textbook=False):
    """RegisterPoints: moves `points` ((n, 3) float32) in place; -> (total, iterations, [step matrices])."""
    total = np.eye(4, dtype=f32)
    steps = []
    done = False
    it = 0
    while not done and it < max_iterations:
        step, _ = icp_step(static, points, good, textbook)
        points[:] = transform_points(points, step)
        done = converged(step, max_t, max_r)[0]
        total = Matrix4x4.Multiply(total, step)
        steps.append(step)
        it += 1
    return total, it, steps


# ---- the bit-exact model: the device's reduction order and csrc/icp_solve.h, operation by operation ----
RED_BLOCKS, RED_THREADS = 256, 256            # the reduction grid of csrc/device_reduce.h: a grid stride of 65536
f64 = np.float64


def _tree256(a):
    """The halving tree over axis 1 (256 entries): s[t] += s[t + o] for t < o, o = 128, 64, ..., 1 -> entry 0."""
    a = a.copy()
    o = 128
    while o > 0:
        a[:, :o] = a[:, :o] + a[:, o:2 * o]
        o //= 2
    return a[:, 0]


def reduce_fixed(values):
    """The sum of `values` ((n,) or (n, K) float64, per column) in the order of the contract: element i is added, in order of i, to
    the accumulator (starting at 0.0) of thread i % 256 of block (i / 256) % 256; a halving tree within each block; then the 256
    block partials, each added to a 0.0 of its own, through the same tree."""
    v = np.asarray(values, f64)
    one = v.ndim == 1
    v = v.reshape(len(v), -1)
    stride = RED_BLOCKS * RED_THREADS
    acc = np.zeros((stride, v.shape[1]), f64)
    with np.errstate(all="ignore"):
        for a in range(0, len(v), stride):
            chunk = v[a:a + stride]
            acc[:len(chunk)] = acc[:len(chunk)] + chunk
        part = _tree256(acc.reshape(RED_BLOCKS, RED_THREADS, -1))       # [block][thread] -> one partial per block
        out = _tree256((0.0 + part)[None])[0]
    return out[0] if one else out


def _pow2_scale(C):
    """pow2_scale of icp_solve.h: the two factors whose product brings the largest |C_ab| into [1, 2)."""
    m = f64(0.0)
    for a in np.abs(C.reshape(-1)):
        if a > m:
            m = a
    f1 = f2 = f64(1.0)
    if not (m > 0.0) or not (m < np.inf):
        return f1, f2
    if m < f64(2.0) ** -1022:
        f1 = f64(2.0) ** 1022
    elif m >= f64(2.0) ** 1023:
        f1 = f64(0.5)
    e = int((np.array(m * f1).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7ff)) - 1023
    f2 = np.array(np.uint64(1023 - e) << np.uint64(52)).view(f64)[()]
    return f1, f2


def kabsch_r_exact(C, info=None):
    """kabsch_r of csrc/icp_solve.h in numpy float64 scalars, one operation per written operation.  `info` (a dict) receives the
    branches taken: sweeps, rotations, zeta_zero (rotations with zeta == 0), ord, s0_zero, rank1 (the cross-product completion), detv, d3."""
    C = np.asarray(C, f64).reshape(3, 3)
    one, zero = f64(1.0), f64(0.0)
    with np.errstate(all="ignore"):
        f1, f2 = _pow2_scale(C)
        W = [[(C[a, b] * f1) * f2 for b in range(3)] for a in range(3)]
        V = [[one if a == b else zero for b in range(3)] for a in range(3)]
        sweeps = rotations = zeta_zero = 0
        for sweep in range(60):
            sweeps += 1
            rotated = False
            for i in range(2):
                for j in range(i + 1, 3):
                    al, be, ga = zero, zero, zero
                    for k in range(3):
                        al = al + W[k][i] * W[k][i]
                        be = be + W[k][j] * W[k][j]
                        ga = ga + W[k][i] * W[k][j]
                    if ga == 0.0 or abs(ga) <= f64(1e-15) * np.sqrt(al * be):
                        continue
                    rotated = True
                    rotations += 1
                    zeta = (be - al) / (f64(2.0) * ga)
                    zeta_zero += int(zeta == 0.0)
                    t = (one if zeta >= 0 else -one) / (abs(zeta) + np.sqrt(one + zeta * zeta))
                    cs = one / np.sqrt(one + t * t)
                    sn = cs * t
                    for k in range(3):
                        wi, wj = W[k][i], W[k][j]
                        W[k][i] = cs * wi - sn * wj
                        W[k][j] = sn * wi + cs * wj
                        vi, vj = V[k][i], V[k][j]
                        V[k][i] = cs * vi - sn * vj
                        V[k][j] = sn * vi + cs * vj
            if not rotated:
                break
        sg = [np.sqrt(W[0][i] * W[0][i] + W[1][i] * W[1][i] + W[2][i] * W[2][i]) for i in range(3)]
        order = [0, 1, 2]
        for i in range(2):
            for j in range(2 - i):
                if sg[order[j]] < sg[order[j + 1]]:
                    order[j], order[j + 1] = order[j + 1], order[j]
        Vs = [[V[k][order[i]] for i in range(3)] for k in range(3)]
        U = [[zero] * 3 for _ in range(3)]
        s0, s1 = sg[order[0]], sg[order[1]]
        rank1 = False
        if s0 == 0.0:
            U = [[one if a == b else zero for b in range(3)] for a in range(3)]
            Vs = [[one if a == b else zero for b in range(3)] for a in range(3)]
        else:
            for k in range(3):
                U[k][0] = W[k][order[0]] / s0
            if s1 > f64(1e-12) * s0:
                for k in range(3):
                    U[k][1] = W[k][order[1]] / s1
            else:
                rank1 = True
                ax, ay, az = abs(U[0][0]), abs(U[1][0]), abs(U[2][0])
                e = [zero, zero, zero]
                e[0 if (ax <= ay and ax <= az) else (1 if ay <= az else 2)] = one
                w = [U[1][0] * e[2] - U[2][0] * e[1], U[2][0] * e[0] - U[0][0] * e[2], U[0][0] * e[1] - U[1][0] * e[0]]
                l = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
                for k in range(3):
                    U[k][1] = w[k] / l
            U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1]
            U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1]
            U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1]
        detv = Vs[0][0] * (Vs[1][1] * Vs[2][2] - Vs[1][2] * Vs[2][1]) - Vs[0][1] * (Vs[1][0] * Vs[2][2] - Vs[1][2] * Vs[2][0]) + \
            Vs[0][2] * (Vs[1][0] * Vs[2][1] - Vs[1][1] * Vs[2][0])
        d3 = one if detv > 0 else (-one if detv < 0 else zero)
        R = np.empty((3, 3), f64)
        for a in range(3):
            for b in range(3):
                R[a, b] = Vs[a][0] * U[b][0] + Vs[a][1] * U[b][1] + d3 * Vs[a][2] * U[b][2]
    if info is not None:
        info.update(sweeps=sweeps, rotations=rotations, zeta_zero=zeta_zero, ord=tuple(order), s0_zero=bool(s0 == 0.0), rank1=rank1, detv=float(detv), d3=float(d3))
    return R


def dist_max_exact(mean, sqsum, n, good):
    """dist_max of icp_solve.h -> (distMax, bracket 0..3, m, sd)."""
    with np.errstate(all="ignore"):
        m, sd, good = f32(mean), f32(np.sqrt(f64(sqsum) / f64(n))), f32(good)
        if m < good:
            return m + f32(3.0) * sd, 0, m, sd
        if m < f32(3.0) * good:
            return m + f32(2.0) * sd, 1, m, sd
        if m < f32(6.0) * good:
            return m + sd, 2, m, sd
        return (m + f32(0.5)) + sd, 3, m, sd


def solve_step_exact(C, pmean, qmean, total_prev, max_t=f32(1e-4), max_r=f32(1e-5), info=None):
    """solve_step of icp_solve.h -> (R f64, step, total, converged): kabsch_r_exact, then Matrix4x4's f32 arithmetic."""
    with np.errstate(all="ignore"):
        R = kabsch_r_exact(C, info)
        rm = np.eye(4, dtype=f32)
        rm[:3, :3] = R.astype(f32)
        _, inv_r = Matrix4x4.Invert(rm)
        pm, qm = np.asarray(pmean, f64).astype(f32), np.asarray(qmean, f64).astype(f32)
        t = Matrix4x4.Transform(pm, inv_r) - qm
        xf = Matrix4x4.Multiply(rm, Matrix4x4.CreateTranslation(t))
        _, step = Matrix4x4.Invert(xf)
        conv = converged(step, f32(max_t), f32(max_r))[0]
        total = Matrix4x4.Multiply(np.asarray(total_prev, f32).reshape(4, 4), step)
    return R, step, total, conv


def icp_step_exact(static, points, total_prev, good=f32(0.01), max_t=f32(1e-4), max_r=f32(1e-5)):
    """One iteration as the device runs it: -> (step, total, converged, details).  `points` is not modified."""
    _, dist, cor = nearest(static, points)
    n = len(dist)
    with np.errstate(all="ignore"):
        d = dist.astype(f64)
        mean = reduce_fixed(d) / f64(n)
        dm = d - mean
        sqsum = reduce_fixed(dm * dm)
        dmax, bracket, m, sd = dist_max_exact(mean, sqsum, n, good)
        keep = dist <= dmax
        p, q = points.astype(f64), cor.astype(f64)
        cols = np.concatenate([np.ones((n, 1)), p, q], axis=1)
        sums = reduce_fixed(np.where(keep[:, None], cols, 0.0))
        pmean, qmean = sums[1:4] / sums[0], sums[4:7] / sums[0]
        pc, qc = p - pmean, q - qmean
        prod = (pc[:, :, None] * qc[:, None, :]).reshape(n, 9)
        C = reduce_fixed(np.where(keep[:, None], prod, 0.0))
    info = {}
    R, step, total, conv = solve_step_exact(C, pmean, qmean, total_prev, max_t, max_r, info)
    info.update(dist_max=dmax, bracket=bracket, mean=m, sd=sd, kept=int(keep.sum()), C=C.reshape(3, 3), pmean=pmean, qmean=qmean, R=R)
    return step, total, conv, info


def register_exact(static, points, max_iterations=100, good=f32(0.01), max_t=f32(1e-4), max_r=f32(1e-5)):
    """sdfk_icp_register bit for bit: moves `points` ((n, 3) float32) in place; -> (total, iterations, [total after each iteration],
    [details of each iteration, "points": the moved points after it])."""
    total = np.eye(4, dtype=f32)
    totals, infos = [], []
    done = False
    it = 0
    while not done and it < max_iterations:
        step, total, done, info = icp_step_exact(static, points, total, good, max_t, max_r)
        with np.errstate(all="ignore"):
            points[:] = transform_points(points, step)
        totals.append(total)
        info["points"] = points.copy()
        infos.append(info)
        it += 1
    return total, it, totals, infos


class NetRandom:
    """System.Random(seed) (seeded: the subtractive generator).  Unverified against .NET here (see the module docstring)."""
    MBIG, MSEED = 2147483647, 161803398

    def __init__(self, seed):
        sa = [0] * 56
        sub = self.MBIG if seed == -2 ** 31 else abs(seed)
        mj = self.MSEED - sub
        sa[55] = mj
        mk = 1
        for i in range(1, 55):
            ii = (21 * i) % 55
            sa[ii] = mk
            mk = mj - mk
            if mk < 0:
                mk += self.MBIG
            mj = sa[ii]
        for _ in range(1, 5):
            for i in range(1, 56):
                sa[i] -= sa[1 + (i + 30) % 55]
                if sa[i] < 0:
                    sa[i] += self.MBIG
        self.sa, self.inext, self.inextp = sa, 0, 21

    def _sample(self):
        self.inext = 1 if self.inext + 1 >= 56 else self.inext + 1
        self.inextp = 1 if self.inextp + 1 >= 56 else self.inextp + 1
        r = self.sa[self.inext] - self.sa[self.inextp]
        if r == self.MBIG:
            r -= 1
        if r < 0:
            r += self.MBIG
        self.sa[self.inext] = r
        return r

    def NextDouble(self):
        return self._sample() * (1.0 / self.MBIG)

    def Next(self, maxValue):
        return int(self.NextDouble() * maxValue)


# ---- the reference's test inputs (Tests/KdTreeTests.cs, Tests/IterativeClosestPointTests.cs) ----
THREE_POINTS = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], f32)
DEG = f32(np.pi) / f32(180.0)   # 1.0f * MathF.PI / 180.0f


def reference_transforms():
    """name -> (points, expected transform, keep) of the six IterativeClosestPointTests cases."""
    M = Matrix4x4
    rx = M.CreateRotationX(f32(1.0) * DEG)
    rxoy = M.Multiply(rx, M.CreateTranslation(0, f32(0.1), 0))
    ozrxoy = M.Multiply(M.Multiply(M.CreateTranslation(0, 0, f32(0.1)), rx), M.CreateTranslation(0, f32(0.1), 0))
    return {
        "ThreePointsOffsetX": (THREE_POINTS, M.CreateTranslation(f32(0.1), 0, 0), 1.0),
        "ThreePointsOffsetXYZ": (THREE_POINTS, M.CreateTranslation(f32(0.1), f32(-0.2), f32(-0.3)), 1.0),
        "ThreePointsRotateY": (THREE_POINTS, M.CreateRotationY(f32(1.0) * DEG), 1.0),
        "ThreePointsRotateXOffsetY": (THREE_POINTS, rxoy, 1.0),
        "ThreePointsOffsetZRotateXOffsetY": (THREE_POINTS, ozrxoy, 1.0),
        "RandomPointsOffsetZRotateXOffsetY": (random_points_100(), ozrxoy, 0.5),
    }


def random_points_100():
    rng = NetRandom(0)
    pts = []
    for _ in range(100):
        x = f32(rng.NextDouble()) - f32(0.5)
        y = f32(rng.NextDouble()) - f32(0.5)
        z = f32(rng.NextDouble()) - f32(0.5)
        pts.append([x, y, z])
    return np.array(pts, f32)


def transform_for_test(points, transform, keep):
    """TransformPoints of the ICP tests: (sources, transformed) with Random(0) deciding which points are kept."""
    rng = NetRandom(0)
    src, out = [], []
    for p in points:
        if rng.NextDouble() < keep:
            src.append(p)
            out.append(Matrix4x4.Transform(p, transform))
    return np.array(src, f32).reshape(-1, 3), np.array(out, f32).reshape(-1, 3)


def check_reference_case(points, expected, keep, register_fn):
    """PointsTest's assertions.  register_fn(static, dynamic) moves `dynamic` in place and returns the total transform."""
    src, moved = transform_for_test(points, expected, keep)
    copy = moved.copy()
    inv = register_fn(points, moved)
    ok, transform = Matrix4x4.Invert(inv)
    assert ok
    np.testing.assert_allclose(transform[3, :3], expected[3, :3], rtol=0, atol=1e-4)
    for k in range(3):
        assert abs(float(expected[k, k]) - float(transform[k, k])) <= 1e-6, (k, expected[k, k], transform[k, k])
    np.testing.assert_allclose(moved, src, rtol=0, atol=1e-4)
    np.testing.assert_allclose(transform_points(copy, inv), src, rtol=0, atol=1e-4)
