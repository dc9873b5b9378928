"""MathF.Sin / Cos / Exp / Log / Atan2 through the other host layers.  C++: builds and runs tests/cpp/mathops_suite.cpp (the gyroid and
the twist written with SdfKit::MathF) and checks what it sampled against the numpy model of the op list it lowered.  C#: the op lists
shim/SdfKit.Hip/Lowering.cs emits for the gyroid and the twist as C# expression trees, transcribed call for call with the
shim's own builder (tests/test_shim_oplists.py: Emitter), compile offline and, replayed through the C ABI, equal the model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sdfkit_amd import _native as N
from tests import mathops_model as M
from tests.test_shim_oplists import Emitter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ADD, SUB, MUL, DIV, NEG, ABS, MIN_SEL, MAX_SEL, MAX_IEEE = 4, 5, 6, 7, 8, 9, 12, 13, 15


def _build(tmp):
    N.lib()  # makes sure libsdfkit_hip.so exists
    exe = os.path.join(tmp, "mathops_suite")
    libdir = os.path.join(ROOT, "sdfkit_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mathops_suite.cpp"), "-o", exe,
                           "-L", libdir, "-lsdfkit_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


# ---- C#: what Lowering.Visitor emits ---------------------------------------------------------------------------------------------
def cs_gyroid():
    """p => new Vector4(0.5f + 0.5f * MathF.Sin(p.X * 4f), 0.5f + 0.5f * MathF.Cos(p.Y * 4f), MathF.Exp(-p.Length()),
                        MathF.Max(MathF.Abs((MathF.Sin(p.X * 4f) * MathF.Cos(p.Y * 4f) + MathF.Sin(p.Y * 4f) * MathF.Cos(p.Z * 4f))
                                            + MathF.Sin(p.Z * 4f) * MathF.Cos(p.X * 4f)) / 4f - 0.08f, p.Length() - 1.2f))"""
    g = Emitter()
    P = {"X": g.X, "Y": g.Y, "Z": g.Z}

    def s4(axis):
        return g.emit(MUL, P[axis], g.const(4.0))

    def trig(op, axis):
        return g.emit(op, s4(axis))
    r = g.emit(ADD, g.const(0.5), g.emit(MUL, g.const(0.5), trig(M.SIN, "X")))
    gg = g.emit(ADD, g.const(0.5), g.emit(MUL, g.const(0.5), trig(M.COS, "Y")))
    b = g.emit(M.EXP, g.emit(NEG, g.length(g.X, g.Y, g.Z)))
    t1 = g.emit(MUL, trig(M.SIN, "X"), trig(M.COS, "Y"))
    t2 = g.emit(MUL, trig(M.SIN, "Y"), trig(M.COS, "Z"))
    t3 = g.emit(MUL, trig(M.SIN, "Z"), trig(M.COS, "X"))
    sheet = g.emit(SUB, g.emit(DIV, g.emit(ABS, g.emit(ADD, g.emit(ADD, t1, t2), t3)), g.const(4.0)), g.const(0.08))
    ball = g.emit(SUB, g.length(g.X, g.Y, g.Z), g.const(1.2))
    w = g.emit(MAX_IEEE, sheet, ball)
    return g.ops, [r, gg, b, w]


def cs_twist():
    """SdfExprEx.ModifyInput(box, p => new Vector3(MathF.Cos(p.Y * 2f) * p.X - MathF.Sin(p.Y * 2f) * p.Z, p.Y,
                                                     MathF.Sin(p.Y * 2f) * p.X + MathF.Cos(p.Y * 2f) * p.Z))
    with the box's colour replaced by (MathF.Atan2(q.Z, q.X), 0, 1) of the twisted point q"""
    g = Emitter()

    def a2():
        return g.emit(MUL, g.Y, g.const(2.0))
    qx = g.emit(SUB, g.emit(MUL, g.emit(M.COS, a2()), g.X), g.emit(MUL, g.emit(M.SIN, a2()), g.Z))
    qz = g.emit(ADD, g.emit(MUL, g.emit(M.SIN, a2()), g.X), g.emit(MUL, g.emit(M.COS, a2()), g.Z))
    q = [qx, g.Y, qz]
    col = g.emit(M.ATAN2, qz, qx)
    zero, one = g.const(0.0), g.const(1.0)
    bnd = [g.const(0.5), g.const(0.9), g.const(0.3)]
    wd = [g.emit(SUB, g.emit(ABS, q[k]), bnd[k]) for k in range(3)]
    z0 = g.const(0.0)
    hi = [g.emit(MAX_SEL, wd[k], z0) for k in range(3)]
    ln = g.length(*hi)
    lo = [g.emit(MIN_SEL, wd[k], z0) for k in range(3)]
    w = g.emit(ADD, ln, g.emit(MAX_IEEE, g.emit(MAX_IEEE, lo[0], lo[1]), lo[2]))
    return g.ops, [col, zero, one, w]


def _arr(ops):
    a = (N.Op * len(ops))()
    for i, (op, x, y, z, w, imm) in enumerate(ops):
        a[i].opcode, a[i].a, a[i].b, a[i].c, a[i].d, a[i].imm = op, x, y, z, w, imm
    return a


def test_cpp_suite_compiles(tmp_path):
    """CPU-side: SdfKit::MathF's transcendentals compile and link against the C ABI."""
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.parametrize("make", [cs_gyroid, cs_twist])
def test_cs_oplists_compile_offline(make):
    ops, out = make()
    assert N.lib().sdfk_program_check(_arr(ops), len(ops), (C.c_int32 * 4)(*out), 1) == 0, N.lib().sdfk_last_error()


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.gpu
def test_cpp_suite_matches_model(tmp_path, gpu):
    exe = _build(str(tmp_path))
    p = subprocess.run(["timeout", "-k", "10", "600", exe, str(tmp_path)], capture_output=True, text=True)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0 and "3 tests, 0 failures" in p.stdout, p.stdout[-3000:]
    for name in ("gyroid", "twist"):
        raw = open(tmp_path / f"{name}.ops", "rb").read()
        n = int(np.frombuffer(raw[:4], np.int32)[0])
        out = [int(v) for v in np.frombuffer(raw[4:20], np.int32)]
        rec = np.frombuffer(raw[20:], np.dtype([("op", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("d", "<i4"), ("imm", "<f4")]))
        assert len(rec) == n
        ops = [(int(r["op"]), int(r["a"]), int(r["b"]), int(r["c"]), int(r["d"]), float(r["imm"])) for r in rec]
        assert sum(o[0] in M.NEW_OPS for o in ops) >= 3, name
        pts = np.fromfile(tmp_path / f"{name}.pts", f32).reshape(-1, 3)
        got = np.fromfile(tmp_path / f"{name}.out", f32).reshape(-1, 4)
        want = M.run(ops, out, pts)
        for k in range(4):
            assert _eq(got[:, k], want[k]), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("make", [cs_gyroid, cs_twist])
def test_cs_oplists_replayed_match_model(gpu, make):
    ops, out = make()
    prog = C.c_void_p()
    N.check(N.lib().sdfk_program_create(_arr(ops), len(ops), (C.c_int32 * 4)(*out), 1, C.byref(prog)))
    try:
        rng = np.random.default_rng(5)
        pts = rng.uniform(-2, 2, (200000, 3)).astype(f32)
        res = np.empty((len(pts), 4), f32)
        N.check(N.lib().sdfk_eval_points(prog, pts.ctypes.data, len(pts), res.ctypes.data))
        want = M.run(ops, out, pts)
        for k in range(4):
            assert _eq(res[:, k], want[k]), k
        mn, mx, small = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), (41, 37, 35)
        vol = C.c_void_p()
        N.check(N.lib().sdfk_volume_create(*small, N.f3(mn), N.f3(mx), 1, C.byref(vol)))
        try:
            N.check(N.lib().sdfk_sample(prog, vol, 0))
            gv, gc = np.empty(small, f32), np.empty(small + (3,), f32)
            N.check(N.lib().sdfk_volume_download(vol, gv.ctypes.data, gc.ctypes.data))
        finally:
            N.lib().sdfk_volume_free(vol)
        wv, wc = M.sample(ops, out, True, mn, mx, *small)
        assert _eq(gv, wv) and _eq(gc, wc)
        assert np.sum(wv < 0) > 100
    finally:
        N.lib().sdfk_program_destroy(prog)
