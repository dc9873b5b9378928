"""numpy model of the INTERVAL form of SDF programs (sdfkit_amd/csrc/sample_codegen.h: sdf_interval, the iv_* functions the block
culling of SDFK_OPT_ELIDE_VOLUME = 2 evaluates over boxes of sample points), op for op what generate_sample_source emits into the
interval body: float32 numpy operations, one rounding each, oracle/ir_interp.py's minimum / maximum.  Written from the comments
and formulas of the header; the five math forms and the two volume forms are the existing models' (tests/mathops_model.py,
tests/voxel_sdf_model.py), called, not copied.

An interval is a pair (lo, hi) of float32 arrays of one shape; NaN in BOTH ends means "unknown" (the whole-interval rule)."""
import numpy as np

from oracle import ir_interp as I
from tests import mathops_model as M
from tests import voxel_sdf_model as VM

f32 = np.float32
INF = f32(np.inf)


def _f(a):
    return np.asarray(a, f32)


def nan_like(a):
    return np.full(np.shape(a), np.nan, f32)


def whole(lo, hi):
    """iv_whole: a NaN end poisons both"""
    lo, hi = _f(lo), _f(hi)
    bad = np.isnan(lo) | np.isnan(hi)
    return np.where(bad, f32(np.nan), lo).astype(f32), np.where(bad, f32(np.nan), hi).astype(f32)


def _poison(bad, r):
    return np.where(bad, f32(np.nan), r[0]).astype(f32), np.where(bad, f32(np.nan), r[1]).astype(f32)


def unknown(a):
    return np.isnan(a[0]) | np.isnan(a[1])


def has_zero(a):
    return (a[0] <= 0) & (a[1] >= 0)


def has_inf(a):
    return np.isinf(a[0]) | np.isinf(a[1])


def make(a, b):
    """iv_make: the box of two coordinates"""
    return I._min_ieee(_f(a), _f(b)), I._max_ieee(_f(a), _f(b))


def iv_add(a, b):
    bad = ((a[1] == INF) & (b[0] == -INF)) | ((a[0] == -INF) & (b[1] == INF))   # inf + -inf somewhere in the box
    return _poison(bad, whole(a[0] + b[0], a[1] + b[1]))


def iv_sub(a, b):
    bad = ((a[1] == INF) & (b[1] == INF)) | ((a[0] == -INF) & (b[0] == -INF))   # inf - inf somewhere in the box
    return _poison(bad, whole(a[0] - b[1], a[1] - b[0]))


def _min4(p):
    return I._min_ieee(I._min_ieee(p[0], p[1]), I._min_ieee(p[2], p[3]))


def _max4(p):
    return I._max_ieee(I._max_ieee(p[0], p[1]), I._max_ieee(p[2], p[3]))


def iv_mul(a, b):
    bad = (has_inf(a) & has_zero(b)) | (has_inf(b) & has_zero(a))               # 0 * inf somewhere in the box
    p = [_f(a[0] * b[0]), _f(a[0] * b[1]), _f(a[1] * b[0]), _f(a[1] * b[1])]
    return _poison(bad, whole(_min4(p), _max4(p)))


def _one_sided(a):
    return (a[0] >= 0) | (a[1] <= 0)


def iv_sqr(a):
    """a * a of ONE value: fl(x * x) is monotone in |x|; zero inside: [0, max]"""
    p0, p1 = _f(a[0] * a[0]), _f(a[1] * a[1])
    return whole(np.where(_one_sided(a), I._min_ieee(p0, p1), f32(0)), I._max_ieee(p0, p1))


def iv_div(a, b):
    bad = (~(b[0] > 0) & ~(b[1] < 0)) | (has_inf(a) & has_inf(b))               # the divisor may be zero or is unknown; inf / inf
    q = [_f(a[0] / b[0]), _f(a[0] / b[1]), _f(a[1] / b[0]), _f(a[1] / b[1])]
    return _poison(bad, whole(_min4(q), _max4(q)))


def iv_neg(a):
    return whole(-a[1], -a[0])


def iv_abs(a):
    x, y = np.abs(a[0]), np.abs(a[1])
    return whole(np.where(_one_sided(a), I._min_ieee(x, y), f32(0)), I._max_ieee(x, y))


def iv_sqrt(a):
    return whole(np.sqrt(a[0]), np.sqrt(a[1]))   # (an end below zero: NaN by itself)


def iv_floor(a):
    return whole(np.floor(a[0]), np.floor(a[1]))


def iv_min(a, b):
    return whole(I._min_ieee(a[0], b[0]), I._min_ieee(a[1], b[1]))


def iv_max(a, b):
    return whole(I._max_ieee(a[0], b[0]), I._max_ieee(a[1], b[1]))


def iv_sel_lt(a, b, c, d):
    """(a < b) ? c : d -- c where a < b for every operand pair, d where for none, else the hull"""
    known = ~unknown(a) & ~unknown(b)
    always = known & (a[1] < b[0])
    never = known & ~always & (a[0] >= b[1])
    lo, hi = whole(I._min_ieee(c[0], d[0]), I._max_ieee(c[1], d[1]))
    lo = np.where(always, c[0], np.where(never, d[0], lo)).astype(f32)
    hi = np.where(always, c[1], np.where(never, d[1], hi)).astype(f32)
    return lo, hi


def _vox(op, vol, ch, X, Y, Z, levels):
    """iv_vox_nearest / iv_vox_linear: the volume model's index maps (vectorised) and its pyramid bound, once per distinct index box;
    the first boxes are compared with the volume model's own scalar form"""
    shape = X[0].shape
    data = VM._channel(vol, ch)
    n, d, mn = data.shape, VM.vol_d(vol), np.asarray(vol[2], f32)
    unk = unknown(X) | unknown(Y) | unknown(Z)
    idx = []
    for a, c in enumerate((X, Y, Z)):
        ends = [np.where(unk, f32(0), e).astype(f32) for e in c]
        if op == VM.NEAREST:
            i0, i1 = (VM.near_idx(VM.quot(e, mn[a], d[a]), n[a]) for e in ends)
        else:
            m = f32(mn[a] + f32(f32(0.5) * d[a]))
            i0, i1 = (VM.lin_i0(VM.lin_u(e, m, d[a], n[a]), n[a]) for e in ends)
            i1 = i1 + (1 if n[a] > 1 else 0)
        idx += [np.ravel(i0), np.ravel(i1)]
    uniq, inv = np.unique(np.stack(idx, -1), axis=0, return_inverse=True)
    bound = np.array([VM.box_bound(data, levels, *(int(v) for v in row)) for row in uniq], f32).reshape(-1, 2)
    inv = np.ravel(inv)
    lo = np.where(np.ravel(unk), f32(np.nan), bound[inv, 0]).astype(f32)
    hi = np.where(np.ravel(unk), f32(np.nan), bound[inv, 1]).astype(f32)
    fl = [np.ravel(c) for c in (*X, *Y, *Z)]
    for i in range(min(len(lo), 24)):
        b = VM.interval(vol, ch, op, (fl[0][i], fl[1][i]), (fl[2][i], fl[3][i]), (fl[4][i], fl[5][i]), levels)
        assert (np.isnan(b[0]) and np.isnan(lo[i])) or (f32(b[0]) == lo[i] and f32(b[1]) == hi[i]), (b, lo[i], hi[i])
    return whole(lo.reshape(shape), hi.reshape(shape))


def pyramids(volumes):
    """the min/max pyramids of every channel of every volume: {(slot, ch): levels}"""
    out = {}
    for s, vol in enumerate(volumes):
        for ch in range(4):
            if ch == 3 or vol[1] is not None:
                out[(s, ch)] = VM.pyramid(VM._channel(vol, ch))
    return out


def interval_all(ops, X, Y, Z, volumes=(), pyr=None):
    """the interval of every value of the program over the boxes X x Y x Z ((lo, hi) pairs of float32 arrays of one shape)"""
    X, Y, Z = ((_f(c[0]), _f(c[1])) for c in (X, Y, Z))
    X, Y, Z = np.broadcast_arrays(*X), np.broadcast_arrays(*Y), np.broadcast_arrays(*Z)
    shape = np.broadcast_shapes(X[0].shape, Y[0].shape, Z[0].shape)
    X, Y, Z = (tuple(np.broadcast_to(e, shape) for e in c) for c in (X, Y, Z))
    if pyr is None and volumes:
        pyr = pyramids(volumes)
    two = {I.ADD: iv_add, I.SUB: iv_sub, I.DIV: iv_div, I.MIN_SEL: iv_min, I.MIN_IEEE: iv_min, I.MAX_SEL: iv_max, I.MAX_IEEE: iv_max}
    one = {I.NEG: iv_neg, I.ABS: iv_abs, I.SQRT: iv_sqrt, I.FLOOR: iv_floor,
           M.SIN: lambda a: M.iv_sin(*a), M.COS: lambda a: M.iv_cos(*a), M.EXP: lambda a: M.iv_exp(*a), M.LOG: lambda a: M.iv_log(*a)}
    v = []
    with np.errstate(all="ignore"):
        for (op, a, b, c, dd, imm) in ops:
            if op == I.CONST: r = (np.full(shape, f32(imm), f32),) * 2
            elif op == I.X: r = X
            elif op == I.Y: r = Y
            elif op == I.Z: r = Z
            elif op == I.MUL: r = iv_sqr(v[a]) if a == b else iv_mul(v[a], v[b])
            elif op in two: r = two[op](v[a], v[b])
            elif op in one: r = one[op](v[a])
            elif op == I.SEL_LT: r = iv_sel_lt(v[a], v[b], v[c], v[dd])
            elif op == M.ATAN2: r = M.iv_atan2(v[a][0], v[a][1], v[b][0], v[b][1])
            elif op in (VM.NEAREST, VM.LINEAR): r = _vox(op, volumes[dd >> 2], dd & 3, v[a], v[b], v[c], pyr[(dd >> 2, dd & 3)])
            else: raise ValueError(op)
            v.append((_f(r[0]), _f(r[1])))
    return v


def interval(ops, out_w, X, Y, Z, volumes=(), pyr=None):
    """sdf_interval: (lo, hi) of the program's distance over the boxes"""
    return interval_all(ops, X, Y, Z, volumes, pyr)[out_w]


# ---- domain-safe random programs ------------------------------------------------------------------------------------------------
def safe_random_program(seed, n_ops=40):
    """A random DAG whose operands are drawn so that most boxes have a KNOWN interval: divisors are abs(..) + c, roots and logarithms
    are taken of abs(..) + c, exponentials of -abs(..), the second operand of atan2 is abs(..) + c (away from the cut).  Returns
    (ops, out_rgbw); every opcode of the volume-less IR appears in the draw."""
    rng = np.random.default_rng(7000 + seed)
    e = (-1, -1, -1, -1)
    ops = [(I.X, *e, 0.0), (I.Y, *e, 0.0), (I.Z, *e, 0.0)]
    for c in rng.choice([0.25, 0.5, 0.75, 1.5, 2.0, 3.0, 0.1, -0.3, -1.25], 4, replace=False):
        ops.append((I.CONST, *e, float(f32(c))))

    def pick():
        k = len(ops)
        return int(rng.integers(max(0, k - 14), k))

    def guarded(i):
        """abs(v_i) + c, c > 0"""
        ops.append((I.ABS, i, -1, -1, -1, 0.0))
        ops.append((I.CONST, *e, float(f32(rng.choice([0.125, 0.5, 1.0])))))
        ops.append((I.ADD, len(ops) - 2, len(ops) - 1, -1, -1, 0.0))
        return len(ops) - 1

    kinds = [I.ADD, I.SUB, I.MUL, "sqr", I.DIV, I.NEG, I.ABS, I.SQRT, I.FLOOR, I.MIN_SEL, I.MAX_SEL, I.MIN_IEEE, I.MAX_IEEE, I.SEL_LT,
             M.SIN, M.COS, M.EXP, M.LOG, M.ATAN2, I.ADD, I.SUB]
    while len(ops) < n_ops:
        op = kinds[int(rng.integers(0, len(kinds)))]
        a, b, c, d = pick(), pick(), pick(), pick()
        if op == "sqr": ops.append((I.MUL, a, a, -1, -1, 0.0))
        elif op == I.DIV: ops.append((op, a, guarded(b), -1, -1, 0.0))
        elif op in (I.SQRT, M.LOG): ops.append((op, guarded(a), -1, -1, -1, 0.0))
        elif op == M.EXP:
            g = guarded(a)
            ops.append((I.NEG, g, -1, -1, -1, 0.0))
            ops.append((op, len(ops) - 1, -1, -1, -1, 0.0))
        elif op == M.ATAN2: ops.append((op, a, guarded(b), -1, -1, 0.0))
        elif op in (I.NEG, I.ABS, I.FLOOR, M.SIN, M.COS): ops.append((op, a, -1, -1, -1, 0.0))
        elif op == I.SEL_LT: ops.append((op, a, b, c, d, 0.0))
        else: ops.append((op, a, b, -1, -1, 0.0))
    k = len(ops)
    return ops, [k - 3, k - 2, k - 4, k - 1]
