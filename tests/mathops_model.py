"""numpy model of MathF.Sin / Cos / Exp / Log / Atan2 in SDF programs (include/sdfkit_hip.h: SDFK_OP_SIN .. SDFK_OP_ATAN2), line for
line the binary64 arithmetic of sdfkit_amd/csrc/mathops.h on float64 / uint64 arrays (so bit for bit the device's and the host's
results), of the interval forms the block culling uses (sample_codegen.h: iv_sin .. iv_atan2), and of whole programs: every other
opcode is evaluated as oracle/ir_interp.py does; the grid sampler, SdfEx.Sample and the ray marcher as tests/voxel_sdf_model.py
models them."""
import types

import numpy as np

from oracle import ir_interp as I
from tests import voxel_sdf_model as VM

f32, f64, u64 = np.float32, np.float64, np.uint64
SIN, COS, EXP, LOG, ATAN2 = 19, 20, 21, 22, 23
NEW_OPS = (SIN, COS, EXP, LOG, ATAN2)
FPI = f32(np.pi)   # (float)pi = 0x40490fdb > pi

H = float.fromhex
TWO_OPI = np.array([0x00000000, 0xa2f9836e, 0x4e441529, 0xfc2757d1, 0xf534ddc0, 0xdb629599, 0x3c439041, 0xfe5163ab, 0xdebbc561,
                    0xb7246e3a], np.uint64)
ATANJ = np.array([0.0] + [H(s) for s in ("0x1.fd5ba9aac2f6ep-4", "0x1.f5b75f92c80ddp-3", "0x1.6f61941e4def1p-2", "0x1.dac670561bb4fp-2",
                                         "0x1.1e00babdefeb4p-1", "0x1.4978fa3269ee1p-1", "0x1.700a7c5784634p-1", "0x1.921fb54442d18p-1")], f64)
TWOOPI, P1, P2, P3 = H("0x1.45f306dc9c883p-1"), H("0x1.921fb548p+0"), H("-0x1.de973dc8p-31"), H("-0x1.9d9cceba3f91fp-62")
PIO2, PI, PI34 = H("0x1.921fb54442d18p+0"), H("0x1.921fb54442d18p+1"), H("0x1.2d97c7f3321d2p+1")
LOG2E, LN2_1, LN2_2, SQRT_HALF = H("0x1.71547652b82fep+0"), H("0x1.62e42fefa3ap-1"), H("-0x1.0ca86c3898dp-49"), H("0x1.6a09e667f3bcdp-1")
SINC = [H(s) for s in ("-0x1.5555555555555p-3", "0x1.1111111111111p-7", "-0x1.a01a01a01a01ap-13", "0x1.71de3a556c734p-19",
                       "-0x1.ae64567f544e4p-26", "0x1.6124613a86d09p-33", "-0x1.ae7f3e733b81fp-41")]
COSC = [H(s) for s in ("-0x1p-1", "0x1.5555555555555p-5", "-0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-16", "-0x1.27e4fb7789f5cp-22",
                       "0x1.1eed8eff8d898p-29", "-0x1.93974a8c07c9dp-37", "0x1.ae7f3e733b81fp-45")]
EXPC = [1.0, 1.0] + [H(s) for s in ("0x1p-1", "0x1.5555555555555p-3", "0x1.5555555555555p-5", "0x1.1111111111111p-7", "0x1.6c16c16c16c17p-10",
                                    "0x1.a01a01a01a01ap-13", "0x1.a01a01a01a01ap-16", "0x1.71de3a556c734p-19", "0x1.27e4fb7789f5cp-22",
                                    "0x1.ae64567f544e4p-26", "0x1.1eed8eff8d898p-29", "0x1.6124613a86d09p-33")]
LOGC = [H(s) for s in ("0x1.5555555555555p-2", "0x1.999999999999ap-3", "0x1.2492492492492p-3", "0x1.c71c71c71c71cp-4", "0x1.745d1745d1746p-4",
                       "0x1.3b13b13b13b14p-4", "0x1.1111111111111p-4", "0x1.e1e1e1e1e1e1ep-5", "0x1.af286bca1af28p-5", "0x1.8618618618618p-5")]
ATANC = [H(s) for s in ("-0x1.5555555555555p-2", "0x1.999999999999ap-3", "-0x1.2492492492492p-3", "0x1.c71c71c71c71cp-4",
                        "-0x1.745d1745d1746p-4", "0x1.3b13b13b13b14p-4", "-0x1.1111111111111p-4")]
M32 = u64(0xffffffff)


def _horner(z, coefs):
    """c0 + z (c1 + z (c2 + ... z c_n)), innermost first, as the header writes it"""
    p = np.full(z.shape, coefs[-1], f64)
    for c in coefs[-2::-1]:
        p = c + z * p
    return p


def _bits(k):
    """sdfk_m_2opi_bits: 32 bits of 2/pi from bit k (int64 array)"""
    p = (k + 31).astype(np.int64)
    w = p >> 5
    two = (TWO_OPI[w] << u64(32)) | TWO_OPI[w + 1]
    return ((two << (p & 31).astype(u64)) >> u64(32)) & M32


def reduce(x):
    """sdfk_m_reduce: (r float64, quad int64) for finite float32 x"""
    x = np.asarray(x, f32)
    xd = x.astype(f64)
    with np.errstate(all="ignore"):
        q = np.rint(xd * TWOOPI)
        r_small = ((xd - q * P1) - q * P2) - q * P3
        quad_small = np.where(np.isfinite(q), q, 0).astype(np.int64) & 3
        big = ~(np.abs(xd) < 2.0 ** 22)
        bits = x.view(np.uint32).astype(u64)
        m = (bits & u64(0x7fffff)) | u64(0x800000)
        s = ((bits >> u64(23)) & u64(0xff)).astype(np.int64) - 151
        s = np.where(big, s, 0)   # (the small path's lanes: any valid window)
        p0 = m * _bits(s + 64)
        p1 = m * _bits(s + 32) + (p0 >> u64(32))
        p2 = m * _bits(s) + (p1 >> u64(32))
        hi = (p2 << u64(32)) | (p1 & M32)
        lo = p0 & M32
        n = (hi + (u64(1) << u64(61))) >> u64(62)
        rh = (hi - (n << u64(62))).view(np.int64)
        r_big = (rh.astype(f64) * 2.0 ** -62 + lo.astype(f64) * 2.0 ** -94) * PIO2
        qn = (n & u64(3)).astype(np.int64)
        neg = x < 0
        r_big = np.where(neg, -r_big, r_big)
        q_big = np.where(neg, (4 - qn) & 3, qn)
    return np.where(big, r_big, r_small), np.where(big, q_big, quad_small)


def sin_poly(r):
    r2 = r * r
    return r + (r * r2) * _horner(r2, SINC)


def cos_poly(r):
    r2 = r * r
    return 1.0 + r2 * _horner(r2, COSC)


def _sincos(x, phase):
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        ok = np.abs(x.astype(f64)) <= H("0x1.fffffep+127")
        r, q = reduce(np.where(ok, x, f32(0)))
        k = (q + phase) & 3
        v = np.where(k & 1, cos_poly(r), sin_poly(r))
        v = np.where(k & 2, -v, v)
        v = np.where(x == 0, f32(1) if phase else x, v.astype(f32))
        return np.where(ok, v, x - x).astype(f32)


def sinf(x): return _sincos(x, 0)
def cosf(x): return _sincos(x, 1)


def expf(x):
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        xd = x.astype(f64)
        k = np.rint(xd * LOG2E)
        r = (xd - k * LN2_1) - k * LN2_2
        p = _horner(r, EXPC)
        mid = (x < f32(89)) & (x > f32(-104))
        v = np.ldexp(p, np.where(mid, k, 0).astype(np.int64)).astype(f32)
        v = np.where(x != x, x + x, np.where(~(x < f32(89)), f32(np.inf), np.where(~(x > f32(-104)), f32(0), v)))
    return v.astype(f32)


def logf(x):
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        m, e = np.frexp(x.astype(f64))
        low = m < SQRT_HALF
        m = np.where(low, m + m, m)
        e = np.where(low, e - 1, e)
        f = m - 1.0
        s = f / (2.0 + f)
        s2 = s * s
        q = _horner(s2, LOGC)
        t = s + s
        ed = e.astype(f64)
        v = (ed * LN2_1 + (ed * LN2_2 + (t + t * (s2 * q)))).astype(f32)
        v = np.where(x == f32(np.inf), x, v)
        v = np.where(x < 0, f32(np.nan), v)
        v = np.where(x == 0, f32(-np.inf), v)
        v = np.where(x != x, x + x, v)
    return v.astype(f32)


def atan2f(y, x):
    y, x = np.broadcast_arrays(np.asarray(y, f32), np.asarray(x, f32))
    with np.errstate(all="ignore"):
        yd, xd = y.astype(f64), x.astype(f64)
        ay, ax = np.abs(yd), np.abs(xd)
        swap = ay > ax
        t = np.where(swap, ax / ay, ay / ax)
        j = np.rint(t * 8.0)
        ji = np.where(np.isfinite(j), j, 0).astype(np.int64).clip(0, 8)
        u = (t * 8.0 - j) / (8.0 + t * j)
        u2 = u * u
        p = _horner(u2, ATANC)
        a = ATANJ[ji] + (u + (u * u2) * p)
        a = np.where(swap, PIO2 - a, a)
        a = np.where(x < 0, PI - a, a)
        both_inf = (ax == np.inf) & (ay == np.inf)
        a = np.where(both_inf, np.where(x > 0, PIO2 / 2, PI34), a)   # (PIO2 / 2: exact, = pi/4 in binary64)
        v = np.where(y < 0, -a, a).astype(f32)
        xneg = np.signbit(x)
        zero = np.where(xneg, np.where(np.signbit(y), -FPI, FPI), y)
        v = np.where(y == 0, zero, v)
        v = np.where((x != x) | (y != y), x + y, v)
    return v.astype(f32)


FUNCS = {SIN: sinf, COS: cosf, EXP: expf, LOG: logf}


# ---- interval forms (sample_codegen.h, kMathPrelude) ----------------------------------------------------------------------------
def succ(v):
    """next float up (+inf and NaN stay; +-0 -> the least subnormal)"""
    v = np.asarray(v, f32)
    b = v.view(np.int32)
    up = np.where(v == 0, np.int32(1), np.where(v > 0, b + 1, b - 1)).astype(np.int32).view(f32)
    return np.where((v == np.inf) | (v != v), v, up).astype(f32)


def pred(v):
    return (-succ(-np.asarray(v, f32))).astype(f32)


def iv_monotone(fn, lo, hi):
    """a faithful f of a nondecreasing function: [pred f(lo), succ f(hi)], NaN when either end is"""
    a, b = pred(fn(lo)), succ(fn(hi))
    bad = (a != a) | (b != b)
    return np.where(bad, f32(np.nan), a).astype(f32), np.where(bad, f32(np.nan), b).astype(f32)


def iv_exp(lo, hi): return iv_monotone(expf, lo, hi)


def iv_log(lo, hi):
    a, b = iv_monotone(logf, lo, hi)
    bad = ~(np.asarray(lo, f32) >= 0)
    return np.where(bad, f32(np.nan), a).astype(f32), np.where(bad, f32(np.nan), b).astype(f32)


def iv_sincos(lo, hi, phase):
    """sin (phase 0) / cos (phase 1) over [lo, hi]: ends +-1 ulp, +1 / -1 where the box may hold a maximum / minimum (position of the
    extremum decided from the reduction, 2^-20 quadrants of slack), clamped to [-1, 1]; width > 4: [-1, 1]; an infinite end: unknown"""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    fn = sinf if phase == 0 else cosf
    with np.errstate(all="ignore"):
        finite = np.isfinite(lo) & np.isfinite(hi)
        l0, h0 = np.where(finite, lo, f32(0)), np.where(finite, hi, f32(0))
        wide = (h0.astype(f64) - l0.astype(f64)) > 4.0
        a, b = fn(l0), fn(h0)
        vlo, vhi = np.minimum(pred(a), pred(b)), np.maximum(succ(a), succ(b))
        rl, ql = reduce(l0)
        rh, qh = reduce(h0)
        tl = rl * (2.0 / np.pi)                       # position of lo within its quadrant, quadrant units
        th = ((qh - ql) & 3).astype(f64) + rh * (2.0 / np.pi)   # position of hi, relative to lo's quadrant centre
        has_max, has_min = np.zeros(lo.shape, bool), np.zeros(lo.shape, bool)
        for jj in range(4):                           # extremum at the centre of quadrant ql + jj
            inside = (tl - 2.0 ** -20 <= jj) & (jj <= th + 2.0 ** -20)
            k = (ql + jj + phase) & 3                 # 1: +1 (sin's quadrant 1), 3: -1
            has_max |= inside & (k == 1)
            has_min |= inside & (k == 3)
        vhi = np.where(has_max | wide, f32(1), np.minimum(vhi, f32(1)))
        vlo = np.where(has_min | wide, f32(-1), np.maximum(vlo, f32(-1)))
        vlo = np.where(finite, vlo, f32(np.nan))
        vhi = np.where(finite, vhi, f32(np.nan))
    return vlo.astype(f32), vhi.astype(f32)


def iv_sin(lo, hi): return iv_sincos(lo, hi, 0)
def iv_cos(lo, hi): return iv_sincos(lo, hi, 1)


def iv_atan2(ylo, yhi, xlo, xhi):
    """corners when the box touches neither the origin nor the cut (x <= 0, y = 0), else [-(float)pi, (float)pi]"""
    ylo, yhi, xlo, xhi = (np.asarray(v, f32) for v in (ylo, yhi, xlo, xhi))
    with np.errstate(all="ignore"):
        c = [atan2f(yy, xx) for yy in (ylo, yhi) for xx in (xlo, xhi)]
        lo = np.minimum(np.minimum(pred(c[0]), pred(c[1])), np.minimum(pred(c[2]), pred(c[3])))
        hi = np.maximum(np.maximum(succ(c[0]), succ(c[1])), np.maximum(succ(c[2]), succ(c[3])))
        cut = (xlo <= 0) & (ylo <= 0) & (yhi >= 0)
        lo = np.where(cut, -FPI, np.maximum(lo, -FPI))
        hi = np.where(cut, FPI, np.minimum(hi, FPI))
        bad = (ylo != ylo) | (yhi != yhi) | (xlo != xlo) | (xhi != xhi)
        lo, hi = np.where(bad, f32(np.nan), lo), np.where(bad, f32(np.nan), hi)
    return lo.astype(f32), hi.astype(f32)


# ---- whole programs ---------------------------------------------------------------------------------------------------------------
def _eval(ops, px, py, pz, volumes=()):
    """every value of the program at the points: ir_interp's semantics (and the volume model's reads) plus the five new opcodes"""
    v = []
    with np.errstate(all="ignore"):
        for (op, a, b, c, dd, imm) in ops:
            if op in FUNCS: r = FUNCS[op](v[a])
            elif op == ATAN2: r = atan2f(v[a], v[b])
            elif op in (VM.NEAREST, VM.LINEAR): r = (VM.nearest if op == VM.NEAREST else VM.linear)(volumes[dd >> 2], dd & 3, v[a], v[b], v[c])
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


def run(ops, out_rgbw, points, volumes=()):
    pts = np.asarray(points, f32)
    v = _eval(ops, np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1]), np.ascontiguousarray(pts[:, 2]), volumes)
    return [v[k] if k >= 0 else None for k in out_rgbw]


def sample(ops, out_rgbw, writes_color, mn, mx, nx, ny, nz, clip=False):
    """Voxels.SampleSdf (+ ClipToBounds): (values, colors)"""
    px, py, pz = VM.grid_points(mn, mx, nx, ny, nz)
    v = _eval(ops, px, py, pz)
    values = v[out_rgbw[3]].copy()
    colors = np.stack([v[out_rgbw[k]] for k in range(3)], -1) if writes_color else np.zeros((nx, ny, nz, 3), f32)
    if clip:
        outside = f32((f32(mx[0]) - f32(mn[0])) / f32(nx))
        values[0], values[-1], values[:, 0], values[:, -1], values[:, :, 0], values[:, :, -1] = (outside,) * 6
    return values, colors


# the ray marcher's arithmetic is tests/voxel_sdf_model.py's, with this module's programs (the same function over other globals)
raymarch = types.FunctionType(VM.raymarch.__code__, dict(VM.__dict__, run=lambda ops, out, pts, vols: run(ops, out, pts, vols)),
                              "raymarch")


def random_program(seed, n_ops=48):
    """oracle.ir_interp.random_program with about one op in four after the inputs and constants replaced by a new one"""
    ops, out = I.random_program(seed, n_ops)
    rng = np.random.default_rng(1000 + seed)
    ops = list(ops)
    for i in range(7, len(ops)):
        a = ops[i][1]
        if rng.random() < 0.25:
            new = int(rng.choice(NEW_OPS))
            ops[i] = (new, a, int(rng.integers(max(0, i - 12), i)) if new == ATAN2 else -1, -1, -1, 0.0)
    return ops, out
