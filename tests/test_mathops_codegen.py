"""CPU checks of MathF.Sin / Cos / Exp / Log / Atan2 in SDF programs (SDFK_OP_SIN .. SDFK_OP_ATAN2): programs with each opcode compile
for gfx950 offline (sdfk_program_check); only programs that use one get the math prelude; the numpy model (tests/mathops_model.py)
is faithful against mpmath on a structured sample and against binary64 libm on millions of strided bit patterns, with special values
exact; the shared arithmetic built as host C++ (tests/cpp/mathops_host.cpp, g++ -ffp-contract=off) equals the model bit for bit;
the model's interval forms contain every point value."""
import ctypes as C
import os
import subprocess

import mpmath
import numpy as np
import pytest

from sdfkit_amd import _native as N
from sdfkit_amd.expr import MathF, Vec3, Vec4, trace
from tests import mathops_model as M
from tests.test_voxel_sdf_codegen import codegen  # noqa: F401  (the code generator built as host C++: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
X, Y, Z = (1, -1, -1, -1, -1, 0.0), (2, -1, -1, -1, -1, 0.0), (3, -1, -1, -1, -1, 0.0)
FMAX = f32(3.4028235e38)


def _arr(ops):
    a = (N.Op * len(ops))()
    for i, (op, x, y, z, w, imm) in enumerate(ops):
        a[i].opcode, a[i].a, a[i].b, a[i].c, a[i].d, a[i].imm = op, x, y, z, w, imm
    return a


def structured():
    """+-0, subnormals, the ends of the ranges, points near multiples of pi/2, near exp / log overflow and underflow, large |x|"""
    v = [0.0, 1e-45, 2e-45, 1.1754942e-38, 1.1754944e-38, 1e-30, 1e-10, 2 ** -12, 0.5, 1.0, 2.0, 10.0, 100.0, 2 ** 22 - 0.5, 2 ** 22,
         2 ** 22 + 1, 1e6, 1e10, 1e20, 1e30, 1e38, float(FMAX), 16367173 * 2.0 ** 72, 88.72283, 88.72284, 88.7229, 88.9, 89.0,
         -87.33654, -87.3366, -103.27893, -103.972, -103.97207, -103.9721, -104.0, 0.99999994, 1.0000001, 0.70710677, 1.4142135]
    v += [k * np.pi / 2 for k in range(1, 200)] + [k * np.pi / 4 for k in range(1, 60)]
    v += list(np.ldexp(1.0, np.arange(-149, 128)))
    v = np.asarray(v, f32)
    with np.errstate(over="ignore"):
        near = [np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))]
    v = np.concatenate([v] + near)
    return np.concatenate([v, -v, np.array([np.inf, -np.inf, np.nan], f32)])


def strided(step=997):
    return np.arange(0, 2 ** 32, step, dtype=np.uint64).astype(np.uint32).view(f32)


def _ord(v):
    i = np.asarray(v, f32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


# ---- code generation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", M.NEW_OPS)
def test_check_compiles_each_op_for_gfx950(op):
    ops = [X, Y, Z, (op, 0, 1 if op == M.ATAN2 else -1, -1, -1, 0.0), (0, -1, -1, -1, -1, 0.25), (4, 3, 4, -1, -1, 0.0)]
    out = (C.c_int32 * 4)(3, 4, 5, 5)
    assert N.lib().sdfk_program_check(_arr(ops), len(ops), out, 1) == 0, N.lib().sdfk_last_error()


def test_check_compiles_a_bound_program_with_math():
    ops = [X, Y, Z, (17, 0, 1, 2, 3, 0.0), (M.SIN, 3, -1, -1, -1, 0.0), (M.ATAN2, 4, 0, -1, -1, 0.0)]
    assert N.lib().sdfk_program_check_bound(_arr(ops), len(ops), (C.c_int32 * 4)(3, 4, 5, 5), 1, 1) == 0, N.lib().sdfk_last_error()


def test_prelude_only_in_programs_that_use_it(codegen):
    ops = [X, Y, Z, (M.COS, 0, -1, -1, -1, 0.0), (M.ATAN2, 1, 2, -1, -1, 0.0), (4, 3, 4, -1, -1, 0.0)]
    (ok, src), (ok2, plain) = codegen([(ops, [-1, -1, -1, 5], 0, 0), (ops[:3] + [(4, 0, 1, -1, -1, 0.0)], [-1, -1, -1, 3], 0, 0)])
    assert ok and ok2
    assert "sdfk_cosf(v0)" in src and "sdfk_atan2f(v1, v2)" in src and "iv_cos(i0)" in src and "iv_atan2(i1, i2)" in src
    assert "struct SdfkK { float k[1]; };" in src
    assert "sdfk_m_reduce" not in plain and "iv_sin" not in plain


def test_tracer_emits_the_opcodes():
    ops, out = trace(lambda p: Vec4.of(Vec3(MathF.Exp(p.x), MathF.Log(p.y), MathF.Atan2(p.z, 1.0)), MathF.Sin(p.x) * MathF.Cos(p.y)), True)
    kinds = [o[0] for o in ops]
    for op in M.NEW_OPS:
        assert op in kinds
    at = ops[kinds.index(M.ATAN2)]
    assert at[1] == 2 and ops[at[2]][0] == 0 and ops[at[2]][5] == 1.0   # (y = p.z, x = the lifted constant)
    with pytest.raises(ValueError):
        MathF.Atan2(1.0, 2.0)


# ---- the model: accuracy and special values ---------------------------------------------------------------------------------------
def _faithful_mp(fn, xs, got):
    """every got within 1 ulp of the exact value (mpmath, 200 bits): count of failures, count not correctly rounded"""
    mpmath.mp.prec = 200
    bad = ncr = 0
    for x, g in zip(xs, got):
        v = fn(x)
        if not mpmath.isfinite(v) or abs(v) > 3.5e38 or (v != 0 and abs(v) < 1e-46):
            continue
        g = f32(g)
        lo, hi = float(np.nextafter(g, f32(-np.inf))), float(np.nextafter(g, f32(np.inf)))
        if not (mpmath.mpf(lo) < v < mpmath.mpf(hi)):
            bad += 1
        elif abs(v) < 3.4e38 and f32(float(v)) != g and abs(mpmath.mpf(float(g)) - v) > abs(mpmath.mpf(float(f32(float(v)))) - v):
            ncr += 1
    return bad, ncr


def test_model_faithful_against_mpmath():
    rng = np.random.default_rng(7)
    xs = np.concatenate([structured(), rng.permutation(strided(4099))[:20000]])
    xs = xs[np.isfinite(xs)]
    for name, fm, fr, dom in [("sin", M.sinf, mpmath.sin, None), ("cos", M.cosf, mpmath.cos, None),
                              ("exp", M.expf, mpmath.exp, None), ("log", M.logf, mpmath.log, lambda x: x > 0)]:
        x = xs if dom is None else xs[dom(xs)]
        bad, ncr = _faithful_mp(lambda t: fr(mpmath.mpf(float(t))), x, fm(x))
        assert bad == 0, name
        print(f"{name}: {len(x)} points, {ncr} not correctly rounded")
    ys = rng.permutation(xs)[:len(xs)]
    pairs = [(y, x) for y, x in zip(ys, xs) if y != 0]   # (mpmath has no signed zero: y = +-0 is test_model_special_values')
    got = M.atan2f(np.array([p[0] for p in pairs], f32), np.array([p[1] for p in pairs], f32))
    bad, _ = _faithful_mp(lambda t: mpmath.atan2(mpmath.mpf(float(t[0])), mpmath.mpf(float(t[1]))), pairs, got)
    assert bad == 0


def test_model_within_one_ulp_of_binary64_on_strided_bits():
    """a few million strided bit patterns against numpy's binary64 functions rounded once (their error, < 2^-52, is far below
    the f32 ulp): 0 results more than 1 ulp away"""
    x = strided()
    x = x[np.isfinite(x)]
    with np.errstate(all="ignore"):
        for fm, fr in ((M.sinf, np.sin), (M.cosf, np.cos), (M.expf, np.exp), (M.logf, np.log)):
            got, want = fm(x), fr(x.astype(f64)).astype(f32)
            both_nan = np.isnan(got) & np.isnan(want)
            assert np.all(both_nan | (np.abs(_ord(got) - _ord(want)) <= 1)), fm.__name__
        y = np.random.default_rng(1).permutation(x)
        got, want = M.atan2f(y, x), np.arctan2(y.astype(f64), x.astype(f64)).astype(f32)
        assert np.all(np.abs(_ord(got) - _ord(want)) <= 1)


def _bits_eq(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))


def test_model_special_values():
    inf, nan, pi = f32(np.inf), f32(np.nan), M.FPI
    z, nz = f32(0.0), f32(-0.0)
    assert _bits_eq(M.sinf([z, nz, inf, -inf, nan]), [z, nz, nan, nan, nan])
    assert _bits_eq(M.cosf([z, nz, inf, -inf, nan]), [1, 1, nan, nan, nan])
    assert _bits_eq(M.expf([-inf, inf, z, nz, 89.0, 100.0, -104.0, -200.0, nan]), [z, inf, 1, 1, inf, inf, z, z, nan])
    assert _bits_eq(M.expf([-103.972, -103.9721]), [f32(1e-45), z])      # the least subnormal and below half of it, correctly rounded
    assert _bits_eq(M.logf([z, nz, f32(-1), -inf, f32(1), inf, nan]), [-inf, -inf, nan, nan, z, inf, nan])
    y = [z, nz, z, nz, z, nz, inf, -inf, inf, -inf, f32(1), f32(-1), f32(1), f32(-1), f32(2), nan, f32(1)]
    x = [z, z, nz, nz, f32(-1), f32(-1), inf, inf, -inf, -inf, z, nz, inf, -inf, f32(5), f32(1), nan]
    want = [z, nz, pi, -pi, pi, -pi, f32(np.pi / 4), f32(-np.pi / 4), f32(3 * np.pi / 4), f32(-3 * np.pi / 4), f32(np.pi / 2),
            f32(-np.pi / 2), z, -pi, f32(np.arctan2(2, 5)), nan, nan]
    assert _bits_eq(M.atan2f(np.array(y, f32), np.array(x, f32)), want)
    assert M.atan2f(f32(3), f32(-1e30)) == pi and float(pi) > np.pi


# ---- the host build of the shared text -------------------------------------------------------------------------------------------
def test_host_build_equals_model(tmp_path):
    exe = str(tmp_path / "mathops_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "mathops_host.cpp"), "-o", exe])
    rng = np.random.default_rng(3)
    a = np.concatenate([structured(), strided(1499)])
    b = np.concatenate([structured()[::-1], rng.permutation(strided(1499))])
    np.stack([a, b], -1).astype(f32).tofile(str(tmp_path / "in"))
    p = subprocess.run([exe, str(tmp_path / "in"), str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "mathops ok" in p.stdout, p.stderr
    host = np.fromfile(str(tmp_path / "out"), f32).reshape(-1, 5)
    for k, want in enumerate((M.sinf(a), M.cosf(a), M.expf(a), M.logf(a), M.atan2f(a, b))):
        assert _bits_eq(host[:, k], want), k


# ---- interval forms -------------------------------------------------------------------------------------------------------------
def _boxes(rng, n):
    lo = np.concatenate([rng.uniform(-20, 20, n), rng.uniform(-3, 3, n), np.ldexp(rng.uniform(1, 2, n), rng.integers(-10, 127, n))
                         * rng.choice([-1, 1], n)]).astype(f32)
    w = np.concatenate([rng.uniform(0, 7, n), rng.uniform(0, 0.5, n), np.zeros(n)]).astype(f32)
    hi = (lo + w).astype(f32)
    hi = np.where(w == 0, np.nextafter(lo, f32(np.inf)), hi).astype(f32)   # 1-ulp boxes (at huge |x|, too)
    k = rng.integers(1, 40, n)                                                  # boxes straddling extrema
    c = (k * (np.pi / 2)).astype(f32)
    return np.concatenate([lo, c - f32(0.01)]).astype(f32), np.concatenate([hi, c + f32(0.01)]).astype(f32)


def _inside(v, lo, hi):
    return np.all(np.isnan(lo) | ((v >= lo) & (v <= hi)))


def test_model_intervals_contain_point_values():
    rng = np.random.default_rng(9)
    lo, hi = _boxes(rng, 1500)
    t = rng.uniform(0, 1, (40, 1))
    pts = np.concatenate([lo[None], hi[None], (lo + (hi.astype(f64) - lo) * t).astype(f32)])
    pts = np.clip(pts, lo, hi).astype(f32)
    for fn, iv in ((M.sinf, M.iv_sin), (M.cosf, M.iv_cos), (M.expf, M.iv_exp), (M.logf, M.iv_log)):
        a, b = iv(lo, hi)
        assert _inside(fn(pts), a, b), fn.__name__
        if fn in (M.sinf, M.cosf):
            assert not np.any(np.isnan(a)) and np.mean(b - a < 1.99) > 0.3   # (known and mostly tighter than [-1, 1])
    ylo, yhi = _boxes(rng, 500)
    xlo = rng.permutation(ylo)
    # boxes touching the cut (x <= 0, y = 0) and the axes
    ylo[:200], yhi[:200] = f32(-0.0), rng.uniform(0, 1, 200).astype(f32)
    ylo[200:300], yhi[200:300] = rng.uniform(-1, 0, 100).astype(f32), f32(0.0)
    xlo[:300] = np.where(np.arange(300) % 2, f32(-1), f32(0.5))
    xhi = (xlo + rng.uniform(0, 2, len(xlo))).astype(f32)
    a, b = M.iv_atan2(ylo, yhi, xlo, xhi)
    for ty in np.linspace(0, 1, 9):
        for tx in np.linspace(0, 1, 9):
            yy = (ylo + (yhi.astype(f64) - ylo) * ty).astype(f32)
            xx = (xlo + (xhi.astype(f64) - xlo) * tx).astype(f32)
            assert _inside(M.atan2f(np.clip(yy, ylo, yhi), np.clip(xx, xlo, xhi)), a, b)
    assert _inside(M.atan2f(f32(-0.0), f32(-1)), a[:1] * 0 - M.FPI, a[:1] * 0 + M.FPI)
    assert np.all((a[:300] == -M.FPI) | (xlo[:300] > 0))


def test_model_interval_unknowns():
    nan = f32(np.nan)
    assert np.isnan(M.iv_log(f32(-1), f32(2))[0]) and not np.isnan(M.iv_log(f32(-0.0), f32(2))[0])
    assert np.isnan(M.iv_sin(f32(1), f32(np.inf))[0]) and np.isnan(M.iv_cos(nan, f32(1))[1])
    assert np.isnan(M.iv_exp(nan, f32(1))[0]) and M.iv_exp(f32(-np.inf), f32(np.inf))[1] == np.inf
    assert M.iv_sin(f32(0), f32(5))[0] == -1 and M.iv_sin(f32(0), f32(5))[1] == 1
