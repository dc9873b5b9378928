"""The interval arithmetic of the block culling (SDFK_OPT_ELIDE_VOLUME = 2: sdf_interval and the iv_* functions of
sdfkit_amd/csrc/sample_codegen.h), checked directly, op by op, on the CPU.

The generated source of a program is cut before `#define SDFK_WRITES_COLOR` (preludes, struct SdfkK, sdf_eval, sdf_interval) and
that SHIPPED text is compiled with g++ behind tests/cpp/interval_shim.h (tests/cpp/interval_host.cpp).  Then
  1. text == tests/interval_model.py, bit for bit (both NaN, or identical bit patterns, signed zeros included);
  2. every point value of the point semantics (oracle/ir_interp.py, tests/mathops_model.py, tests/voxel_sdf_model.py) inside a box
     with a known interval lies in it, and is not NaN;
  3. on the boxes sdfk_cull_blocks forms on real grids the model interval contains the sampled volume's [min, max] per box;
  4. per-opcode edge tables, written out below;
  5. single textual mutations of the test's copy of the text are each detected by 1 or 2."""
import concurrent.futures
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from oracle import ir_interp as I
from sdfkit_amd.api import _box_distance
from sdfkit_amd.expr import MathF, Vec4, trace, trace_bound
from tests import interval_model as IM
from tests import mathops_model as M
from tests import scenes
from tests import voxel_sdf_model as VM
from tests.test_voxel_sdf_codegen import codegen  # noqa: F401  (the code generator built as host C++: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
E = (-1, -1, -1, -1)
OPX, OPY, OPZ = (I.X, *E, 0.0), (I.Y, *E, 0.0), (I.Z, *E, 0.0)
FMAX = f32(3.4028235e38)
INF = f32(np.inf)
TINY = f32(1e-45)


def bits_eq(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- programs -------------------------------------------------------------------------------------------------------------------
def _sphere_volume(n, mn, mx, colors, seed):
    """a smooth field with a zero level (the distance of a sphere of radius 0.9, sampled), colours random"""
    px, py, pz = VM.grid_points(mn, mx, *n)
    vals = (np.sqrt(px * px + py * py + pz * pz) - f32(0.9)).astype(f32)
    cols = np.random.default_rng(seed).uniform(0, 1, tuple(n) + (3,)).astype(f32) if colors else None
    return (vals, cols, mn, mx)


def _random_volume(n, mn, mx, colors, seed, bad=None):
    rng = np.random.default_rng(seed)
    vals = rng.uniform(-1, 1, n).astype(f32)
    if bad is not None:
        vals[bad] = np.inf
    cols = rng.uniform(0, 1, tuple(n) + (3,)).astype(f32) if colors else None
    return (vals, cols, mn, mx)


def bound_scenes():
    """the bound scenes of tests/test_gpu_voxel_sdf.py (two volumes with colours; a volume read united with a box, through both
    index maps) over model volumes: smooth fields, so that the culling has something to decide"""
    v0 = _sphere_volume((9, 1, 13), (-1.0, -0.25, -1.5), (1.25, 0.5, 1.0), True, 1)     # an N = 1 axis
    v1 = _sphere_volume((12, 10, 14), (-1.5, -1.0, -1.25), (1.0, 1.5, 1.25), True, 2)
    vm = _sphere_volume((40, 36, 44), (-1.25,) * 3, (1.25,) * 3, False, 3)

    def two(p):
        c = [p.x.b.voxel(VM.LINEAR, v1, p, ch) for ch in range(2)]
        g = p.x.b.voxel(VM.NEAREST, v0, p, 1)
        return Vec4(c[0], c[1], g, p.x.b.voxel(VM.NEAREST, v0, p, 3) + p.x.b.voxel(VM.LINEAR, v1, p, 3) * 0.5)

    def union(interpolate):
        def fn(p):
            a = p.x.b.voxel(VM.LINEAR if interpolate else VM.NEAREST, vm, p, 3)
            return Vec4.of((1.0, 1.0, 1.0), MathF.Min(a, _box_distance(p.__class__(p.x - 0.75, p.y, p.z), (0.4, 0.3, 0.5))))
        return fn
    res = []
    for name, fn in (("bound_two_volumes", two), ("bound_union_nearest", union(False)), ("bound_union_linear", union(True))):
        ops, out, vols = trace_bound(fn, True)
        res.append(dict(name=name, ops=ops, out=out, wc=1, vols=vols))
    return res


def mathops_scenes():
    from tests.test_gpu_mathops import SCENES
    return [dict(name=k, ops=o[0], out=o[1], wc=1, vols=[]) for k, o in ((k, trace(fn, True)) for k, fn in SCENES.items())]


def catalogue_scenes():
    res = []
    for name, mk in scenes.CATALOGUE.items():
        _, sdf = mk()
        ops, out = trace(sdf.fn, sdf.writes_color)
        res.append(dict(name=name, ops=ops, out=out, wc=int(sdf.writes_color), vols=[]))
    return res


N_SAFE = 12


def whole_programs():
    res = catalogue_scenes() + mathops_scenes()
    res += [dict(name=f"random_{s}", ops=o[0], out=o[1], wc=1, vols=[]) for s, o in ((s, I.random_program(s)) for s in range(24))]
    res += [dict(name=f"mrandom_{s}", ops=o[0], out=o[1], wc=1, vols=[]) for s, o in ((s, M.random_program(s)) for s in range(8))]
    res += [dict(name=f"safe_{s}", ops=o[0], out=o[1], wc=1, vols=[]) for s, o in ((s, IM.safe_random_program(s)) for s in range(N_SAFE))]
    return res + bound_scenes()


# volumes of the edge tables: dimensions 1 and 2, 13 x 6 x 21 with a non-finite voxel and colours, a power of two
EDGE_VOLS = [_random_volume((1, 2, 5), (-1.0, -0.5, 0.0), (1.0, 0.5, 2.0), False, 11),
             _random_volume((13, 6, 21), (-1.0, -0.5, -2.0), (1.0, 0.5, 2.0), True, 12, bad=(6, 3, 10)),
             _random_volume((16, 8, 4), (0.0, 0.0, 0.0), (4.0, 2.0, 1.0), False, 13)]


def _poisoned_volume():
    """65 x 33 x 17 with colours (rows of 17 are padded to 20): +inf in the first voxel, NaN in the last one -- the clipped corner cell
    of every level -- and -inf inside; a NaN in colour channel 1 somewhere else"""
    vals, cols, mn, mx = _random_volume((65, 33, 17), (-2.0, -1.0, -0.5), (2.0, 1.0, 0.5), True, 24)
    vals[0, 0, 0], vals[64, 32, 16], vals[40, 8, 3] = np.inf, np.nan, -np.inf
    cols[10, 20, 5, 1] = np.nan
    return (vals, cols, mn, mx)


def _one_nan_volume():
    """64 x 64 x 64, a power of two, with one NaN: its ancestors are poisoned at every level, and no other cell"""
    vol = _random_volume((64, 64, 64), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), False, 25)
    vol[0][37, 21, 50] = np.nan
    return vol


def _big_volume():
    """176 x 160 x 160: level 1 has 88 x 80 x 80 = 563 200 cells, more than the 2048 x 256 lanes k_vol_pyr_base is launched with, so
    the cells from x = 164 on are the second step of its grid stride.  A smooth field, distinct from voxel to voxel, and two
    non-finite voxels, one of them in the second step."""
    n, mn, mx = (176, 160, 160), (-1.1, -1.0, -1.0), (1.1, 1.0, 1.0)
    px, py, pz = VM.grid_points(mn, mx, *n)
    vals = (np.sqrt(px * px + py * py + pz * pz) - f32(0.9) + f32(0.0625) * px * py + f32(0.03125) * pz).astype(f32)
    vals[170, 100, 33], vals[5, 150, 150] = np.nan, -np.inf
    return (vals, None, mn, mx)


# the smallest shapes at which a level of the min/max pyramid can go wrong: no pyramid at all (nlev == 0); 257 x 3 x 5, whose x cells
# run 129, 65, 33, 17, 9, 5, 3, 2, 1 (a clipped last cell at every level) while y and z collapse early; an N = 1 and an N = 2 axis
# with a long z; the three above.  BIG_VOL gets a handful of boxes instead of a vox_table.
EDGE_VOLS += [_random_volume((1, 1, 1), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), False, 21),
              _random_volume((257, 3, 5), (-2.0, -0.5, -1.0), (2.0, 0.5, 1.0), False, 22),
              _random_volume((2, 1, 64), (-0.5, -0.25, -2.0), (0.5, 0.25, 2.0), False, 23),
              _poisoned_volume(), _one_nan_volume(), _big_volume()]
POISONED_VOL, BIG_VOL = 6, 8
assert EDGE_VOLS[POISONED_VOL][0].shape == (65, 33, 17) and EDGE_VOLS[BIG_VOL][0].shape == (176, 160, 160)


def single_op_programs():
    """one program per opcode: the operands are X, Y, Z or constants, so that the box IS the operand interval"""
    P = {}
    for name, op in (("add", I.ADD), ("sub", I.SUB), ("mul", I.MUL), ("div", I.DIV), ("min_sel", I.MIN_SEL), ("max_sel", I.MAX_SEL),
                     ("min_ieee", I.MIN_IEEE), ("max_ieee", I.MAX_IEEE), ("atan2", M.ATAN2)):
        P[name] = [OPX, OPY, OPZ, (op, 0, 1, -1, -1, 0.0)]
    P["sqr"] = [OPX, OPY, OPZ, (I.MUL, 0, 0, -1, -1, 0.0)]
    for name, op in (("neg", I.NEG), ("abs", I.ABS), ("sqrt", I.SQRT), ("floor", I.FLOOR), ("sin", M.SIN), ("cos", M.COS),
                     ("exp", M.EXP), ("log", M.LOG)):
        P[name] = [OPX, OPY, OPZ, (op, 0, -1, -1, -1, 0.0)]
    P["sel_lt"] = [OPX, OPY, OPZ, (I.CONST, *E, 7.0), (I.SEL_LT, 0, 1, 2, 3, 0.0)]
    P["const"] = [OPX, OPY, OPZ, (I.CONST, *E, -0.0), (I.CONST, *E, 2.5), (I.MUL, 0, 4, -1, -1, 0.0), (I.ADD, 5, 3, -1, -1, 0.0)]
    res = [dict(name="op_" + k, ops=v, out=[-1, -1, -1, len(v) - 1], wc=0, vols=[]) for k, v in P.items()]
    for vi, vol in enumerate(EDGE_VOLS):
        for nm, op in (("nearest", VM.NEAREST), ("linear", VM.LINEAR)):
            for ch in ((3, 1) if vol[1] is not None else (3,)):
                ops = [OPX, OPY, OPZ, (op, 0, 1, 2, ch, 0.0)]
                res.append(dict(name=f"op_vox_{nm}_{vi}_{ch}", ops=ops, out=[-1, -1, -1, 3], wc=0, vols=[vol]))
    return res


# ---- the shipped text as a host program ---------------------------------------------------------------------------------------
def cut(src, ops):
    """(preludes, struct SdfkK .. sdf_interval, number of K.k slots, the constants in slot order) of a generated source"""
    i, j = src.index("struct SdfkK"), src.index("#define SDFK_WRITES_COLOR")
    pre, body = src[:i], src[i:j]
    nk = int(re.search(r"struct SdfkK \{ float k\[(\d+)\]", body).group(1))
    ibody = body[body.index("sdf_interval("):]
    # the parameter order is read off the text: slot n holds the constant of the op whose interval is iv_const(K.k[n])
    slots = {int(n): int(op) for op, n in re.findall(r"const sdfk_iv i(\d+) = iv_const\(K\.k\[(\d+)\]\);", ibody)}
    assert sorted(slots) == list(range(len(slots))) and len(slots) <= nk
    k = [ops[slots[n]][5] for n in range(len(slots))]
    return pre, body, nk, np.asarray(k + [0.0] * (nk - len(k)), f32)


class Text:
    """the cut sources of a list of programs, and translation units made of them"""

    def __init__(self, codegen, programs):
        self.programs = programs
        res = codegen([(p["ops"], p["out"], p["wc"], len(p["vols"])) for p in programs])
        self.cuts = []
        for p, (ok, src) in zip(programs, res):
            assert ok, (p["name"], src)
            self.cuts.append(cut(src, p["ops"]))
        pres = [c[0] for c in self.cuts]
        self.base = min(pres, key=len)
        assert "SDFK_M_FN" not in self.base and "SdfkVol" not in self.base and all(q.startswith(self.base) for q in pres)
        self.math = next((q[len(self.base):] for q in pres if "SDFK_M_FN" in q and "SdfkVol" not in q), "")
        self.vol = next((q[len(self.base):] for q in pres if "SDFK_M_FN" not in q and "SdfkVol" in q), "")
        for q in pres:   # every program's preludes are these pieces, in this order
            assert q == self.base + (self.math if "SDFK_M_FN" in q else "") + (self.vol if "SdfkVol" in q else "")

    def unit(self, mutate=None):
        t = self.base + self.math + self.vol
        for n, (p, c) in enumerate(zip(self.programs, self.cuts)):
            t += f"namespace p{n} {{\n{c[1]}INTERVAL_RUN({c[2]}, {'K.V = (const SdfkVol*)V;' if p['vols'] else ''})\n}}\n"
        t += "static const interval_run_fn kPrograms[] = {" + ", ".join(f"p{n}::run" for n in range(len(self.programs))) + "};\n"
        if mutate:
            m = mutate(t)
            assert m != t, "the mutation did not apply"
            t = m
        return t

    def build(self, d, tag, mutate=None):
        inc, exe = os.path.join(d, f"programs_{tag}.inc"), os.path.join(d, f"interval_{tag}")
        open(inc, "w").write(self.unit(mutate))
        # (no FMA contraction, as lib_jit.hip asks of hiprtc with -ffp-contract=off; it compiles at -O3, g++ here at -O2)
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DSDFK_KERNELS=0x200", f'-DINTERVAL_PROGRAMS="{inc}"']
        if self.vol:
            cmd.append("-DINTERVAL_HAS_VOLUMES")
        subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpp", "interval_host.cpp"), "-o", exe])
        return exe


_RECORDS = {}


def volume_record(vol, padding="nan"):
    """the record of a volume.  Rows are padded as the device lays them out; nobody may read the padding: it is NaN, or (padding ==
    "fmax") alternately +FMAX and -FMAX, which a minimum or maximum that wrongly reads it cannot lose the way it loses a NaN."""
    key = (id(vol), padding)
    if key in _RECORDS and _RECORDS[key][0] is vol:
        return _RECORDS[key][1]
    vals, cols, mn, _ = vol
    n = vals.shape
    pitch = (n[2] + 3) & ~3

    def padded(shape):
        if padding == "nan":
            return np.full(shape, np.nan, f32)
        return np.where(np.arange(int(np.prod(shape))) % 2 == 0, FMAX, -FMAX).astype(f32).reshape(shape)
    d = VM.vol_d(vol)
    m = (np.asarray(mn, f32) + (f32(0.5) * d).astype(f32)).astype(f32)
    lv = VM.pyramid(vals)
    pv = padded(n[:2] + (pitch,))
    pv[..., :n[2]] = vals
    b = struct.pack("<6i", *n, pitch, int(cols is not None), len(lv) - 1)
    b += np.concatenate([np.asarray(mn, f32), d, m]).astype(f32).tobytes() + pv.tobytes()
    if cols is not None:
        pc = padded(n[:2] + (pitch, 3))
        pc[..., :n[2], :] = cols
        b += pc.tobytes()
    for ch in (range(4) if cols is not None else (3,)):
        for lo, hi in (lv if ch == 3 else VM.pyramid(VM._channel(vol, ch)))[1:]:
            b += struct.pack("<i", lo.size) + np.stack([lo, hi], -1).astype(f32).tobytes()
    _RECORDS[key] = (vol, b)   # (the volumes are module constants, written once per build that is run)
    return b


def write_records(path, recs, with_volumes=True, padding="nan"):
    """recs: (program index, constants, volumes, boxes [n, 6], points [m, 3])"""
    with open(path, "wb") as f:
        for prog, k, vols, boxes, pts in recs:
            f.write(struct.pack("<5i", prog, len(k), len(vols) if with_volumes else 0, len(boxes), len(pts)))
            f.write(np.asarray(k, f32).tobytes())
            for v in (vols if with_volumes else ()):
                f.write(volume_record(v, padding))
            f.write(np.ascontiguousarray(boxes, f32).tobytes() + np.ascontiguousarray(pts, f32).tobytes())


def read_results(path, recs):
    data, o, res = np.fromfile(path, f32), 0, []
    for _, _, _, boxes, pts in recs:
        nb, npt = len(boxes), len(pts)
        res.append((data[o:o + 2 * nb].reshape(nb, 2), data[o + 2 * nb:o + 2 * nb + npt]))
        o += 2 * nb + npt
    assert o == len(data)
    return res


def run_host(exe, d, tag, recs):
    src, dst = os.path.join(d, f"in_{tag}"), os.path.join(d, f"out_{tag}")
    write_records(src, recs)
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "interval ok" in p.stdout, p.stderr
    return read_results(dst, recs)


# ---- boxes ----------------------------------------------------------------------------------------------------------------------
def ivs(pairs):
    a = np.asarray(pairs, f32).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy()


SPECIALS = np.array([-np.inf, -FMAX, -2.0 ** 23, -100.0, -3.0, -1.0, -0.5, -1e-30, -1e-45, -0.0, 0.0, 1e-45, 1.1754944e-38, 1e-30, 0.5, 1.0,
                     2.0, 3.0, 100.0, 2.0 ** 23, 1e30, 2e30, FMAX, np.inf], f32)


def special_intervals():
    """every [a, b], a <= b, of the special values: signed zeros and infinities as ends, boxes through zero, degenerate boxes"""
    i, j = np.triu_indices(len(SPECIALS))
    return SPECIALS[i], SPECIALS[j]


def ulp_boxes():
    """1-ulp boxes at every binade, both signs, on both sides of the power of two"""
    p = np.ldexp(f32(1), np.arange(-149, 128)).astype(f32)
    lo = np.concatenate([p, M.pred(p)])
    hi = np.concatenate([M.succ(p), p])
    return np.concatenate([lo, -hi]), np.concatenate([hi, -lo])


def cross(a, b):
    """all pairs of two interval lists"""
    ia, ib = np.meshgrid(np.arange(len(a[0])), np.arange(len(b[0])), indexing="ij")
    return (a[0][ia.ravel()], a[1][ia.ravel()]), (b[0][ib.ravel()], b[1][ib.ravel()])


def cat(*lists):
    return np.concatenate([l[0] for l in lists]).astype(f32), np.concatenate([l[1] for l in lists]).astype(f32)


def boxes6(X, Y=None, Z=None):
    n = len(X[0])
    zero = (np.zeros(n, f32), np.zeros(n, f32))
    Y, Z = Y or zero, Z or zero
    return np.stack([X[0], X[1], Y[0], Y[1], Z[0], Z[1]], -1).astype(f32)


def axis_points(lo, hi, dense=0):
    """candidate coordinates inside [lo, hi], per box: [k, n].  The ends, their inner neighbours, the midpoint, +0 and -0 where the
    box holds them (-0 is not inside [+0, b], nor +0 inside [a, -0]: iv_make orders the zeros), `dense` evenly spaced ones."""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    with np.errstate(all="ignore"):
        mid = (lo.astype(f64) / 2 + hi.astype(f64) / 2).astype(f32)
        mid = np.where(np.isfinite(mid), mid, lo)
        c = [lo, hi, np.minimum(M.succ(lo), hi), np.maximum(M.pred(hi), lo), np.clip(mid, lo, hi)]
        zin = (lo <= 0) & (hi >= 0)
        c.append(np.where(zin & ~((hi == 0) & np.signbit(hi)), f32(0.0), lo))
        c.append(np.where(zin & ~((lo == 0) & ~np.signbit(lo)), f32(-0.0), lo))
        fin = np.isfinite(lo) & np.isfinite(hi)
        for t in np.linspace(0, 1, dense + 2)[1:-1] if dense else ():
            v = (lo.astype(f64) + (hi.astype(f64) - lo.astype(f64)) * t).astype(f32)
            c.append(np.where(fin, np.clip(v, lo, hi), lo))
    return np.stack(c).astype(f32)


def all_floats(lo, hi, limit=64):
    """every float of [lo, hi] when there are at most `limit` (finite ends of one sign or zero), else None"""
    o0, o1 = int(M_ord(lo)), int(M_ord(hi))
    if not (np.isfinite(lo) and np.isfinite(hi)) or o1 - o0 >= limit:
        return None
    o = np.arange(o0, o1 + 1, dtype=np.int64)
    v = np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(f32)
    if o0 <= 0 <= o1:   # both zeros, where the box holds them
        z = [s for s in (f32(0.0), f32(-0.0)) if not (s.view(np.uint32) == 0 and hi == 0 and np.signbit(hi)) and
             not (s.view(np.uint32) != 0 and lo == 0 and not np.signbit(lo))]
        v = np.concatenate([v[v != 0], np.asarray(z, f32)])
    return v.astype(f32)


def M_ord(v):
    i = np.asarray(v, f32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def box_points(B, dense=0):
    """[k, n, 3] sample points of boxes B [n, 6]: the product of the per-axis candidates (an axis of width 0 contributes one)"""
    ax = []
    for a in range(3):
        lo, hi = B[:, 2 * a], B[:, 2 * a + 1]
        ax.append(axis_points(lo, hi, dense) if np.any(lo.view(np.uint32) != hi.view(np.uint32)) else lo[None])
    gx, gy, gz = np.meshgrid(*(np.arange(len(a)) for a in ax), indexing="ij")
    return np.stack([ax[0][gx.ravel()], ax[1][gy.ravel()], ax[2][gz.ravel()]], -1)


def contained(v, lo, hi):
    """assertion 2, per box: every point value [k, n] lies in the known interval and none is NaN; unknown boxes pass"""
    with np.errstate(invalid="ignore"):
        ok = (v >= lo) & (v <= hi)
    return np.isnan(lo) | np.all(ok, axis=0)


def point_values(p, pts):
    """the point semantics at pts [..., 3]"""
    pts = np.asarray(pts, f32)
    v = M._eval(p["ops"], np.ascontiguousarray(pts[..., 0]), np.ascontiguousarray(pts[..., 1]), np.ascontiguousarray(pts[..., 2]), p["vols"])
    return v[p["out"][3]]


def model_interval(p, B, pyr=None):
    return IM.interval(p["ops"], p["out"][3], (B[:, 0], B[:, 1]), (B[:, 2], B[:, 3]), (B[:, 4], B[:, 5]), p["vols"], pyr)


# ---- the culler's boxes -------------------------------------------------------------------------------------------------------
def grid_axes(mn, mx, dims):
    """the coordinates sdfk_coord forms: m + (float)i * d per axis (Voxels.cs:81,104-106)"""
    mn, mx = np.asarray(mn, f32), np.asarray(mx, f32)
    d = ((mx - mn) / np.array(dims, f32)).astype(f32)
    m = (mn + f32(0.5) * d).astype(f32)
    return [(m[a] + (np.arange(dims[a], dtype=f32) * d[a]).astype(f32)).astype(f32) for a in range(3)]


def culler_index_boxes(dims):
    """(sub, coarse): per axis (first index, last index) arrays of the 8 x 4 x 4 sub-boxes of whole blocks and of the 128 x 8 x 8
    coarse boxes, clamped at the upper faces, as sdfk_cull_blocks forms them"""
    nx, ny, nz = dims
    sub = [(8 * np.arange((nx // 64) * 8), 8 * np.arange((nx // 64) * 8) + 7)] + [(4 * np.arange(n // 4), 4 * np.arange(n // 4) + 3) for n in (ny, nz)]
    nb = [(nx + 63) // 64, (ny + 3) // 4, (nz + 3) // 4]
    coarse = []
    for a, w in enumerate((128, 8, 8)):
        i0 = w * np.arange((nb[a] + 1) >> 1)
        coarse.append((i0, np.minimum(i0 + w - 1, dims[a] - 1)))
    return sub, coarse


def culler_boxes(mn, mx, dims):
    """(the axes' coordinates, sub, coarse) of a grid"""
    return (grid_axes(mn, mx, dims), *culler_index_boxes(dims))


def axis_boxes(ax, idx):
    """iv_make of the coordinates of the first and last index, per axis, broadcastable to [x, y, z]"""
    out = []
    for a in range(3):
        lo, hi = IM.make(ax[a][idx[a][0]], ax[a][idx[a][1]])
        shp = [1, 1, 1]
        shp[a] = -1
        out.append((lo.reshape(shp), hi.reshape(shp)))
    return out


def sample_volume(p, ax):
    """the program at every sample point, in slabs of x"""
    nx, ny, nz = (len(a) for a in ax)
    W = np.empty((nx, ny, nz), f32)
    for x0 in range(0, nx, 8):
        px = ax[0][x0:x0 + 8, None, None] + np.zeros((1, ny, nz), f32)
        py = ax[1][None, :, None] + np.zeros(px.shape, f32)
        pz = ax[2][None, None, :] + np.zeros(px.shape, f32)
        W[x0:x0 + 8] = M._eval(p["ops"], px, py, pz, p["vols"])[p["out"][3]]
    return W


def box_extremes(W, idx):
    """(min, max, any NaN) of W over the boxes idx (first indices per axis; the boxes tile from there to the next start or the end)"""
    mn, mx, bad = W, W, np.isnan(W)
    for a in range(3):
        st = idx[a][0]
        ln = idx[a][1] - idx[a][0] + 1
        k = st[-1] + ln[-1]   # (sub-boxes stop at the last whole block)
        sl = [slice(None)] * 3
        sl[a] = slice(0, k)
        mn, mx, bad = (np.fmin.reduceat(mn[tuple(sl)], st, axis=a), np.fmax.reduceat(mx[tuple(sl)], st, axis=a),
                       np.logical_or.reduceat(bad[tuple(sl)], st, axis=a))
    return mn, mx, bad


GRIDS = [(136, 132, 128), (300, 236, 250)]


def scene_bounds(p):
    if p["name"] in ("gyroid", "twist", "polar", "smooth_union") or p["name"].startswith("bound_"):
        return [-1.5] * 3, [1.5] * 3          # tests/test_gpu_mathops.py: BOX; tests/test_gpu_voxel_sdf.py
    return [-2.8125] * 3, [2.8125] * 3        # tests/test_gpu_elide_volume.py


_SCENES = None


def _scene_list():
    global _SCENES
    if _SCENES is None:
        _SCENES = catalogue_scenes() + mathops_scenes() + bound_scenes()
    return _SCENES


def check_culler_chunk(task):
    """assertion 3 for one scene, grid and column of coarse boxes (x rows [x0, x1), x0 a multiple of 128: the sub-boxes and coarse
    boxes of the column are those of a grid of x1 - x0 rows at these coordinates): {kind: (boxes decided at iso 0, boxes)}"""
    si, dims, x0, x1 = task
    p = _scene_list()[si]
    mn, mx = scene_bounds(p)
    ax = grid_axes(mn, mx, dims)
    ax = [ax[0][x0:x1], ax[1], ax[2]]
    sub, coarse = culler_index_boxes((x1 - x0, dims[1], dims[2]))
    W = sample_volume(p, ax)
    pyr = IM.pyramids(p["vols"]) if p["vols"] else None
    counts = {}
    for kind, idx in (("sub", sub), ("coarse", coarse)):
        if any(len(i[0]) == 0 for i in idx):
            counts[kind] = (0, 0)
            continue
        X, Y, Z = axis_boxes(ax, idx)
        lo, hi = IM.interval(p["ops"], p["out"][3], X, Y, Z, p["vols"], pyr)
        vmin, vmax, bad = box_extremes(W, idx)
        assert lo.shape == vmin.shape
        known = ~np.isnan(lo)
        assert not np.any(bad & known), (p["name"], dims, x0, kind, "a NaN voxel inside a box with a known interval", np.argwhere(bad & known)[:3])
        with np.errstate(invalid="ignore"):
            ok = ~known | ((lo <= vmin) & (vmax <= hi))
        assert np.all(ok), (p["name"], dims, x0, kind, np.argwhere(~ok)[:3])
        with np.errstate(invalid="ignore"):
            counts[kind] = (int(np.sum(known & ((lo > 0) | (hi <= 0)))), lo.size)
    return si, dims, counts


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole(codegen, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("interval_whole"))
    t = Text(codegen, whole_programs())
    return t, t.build(d, "whole"), d


@pytest.fixture(scope="module")
def single(codegen, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("interval_single"))
    t = Text(codegen, single_op_programs())
    return t, t.build(d, "single"), d


def test_host_sqrt_is_correctly_rounded(single):
    """the shim's sdfk_sqrt (one lane: short path for [2^-96, FLT_MAX], __builtin_sqrtf otherwise) is the binary64 root rounded once,
    on every power of two, its neighbours, a few thousand strided bit patterns and the special values"""
    _, exe, d = single
    p = np.ldexp(f32(1), np.arange(-149, 128)).astype(f32)
    x = np.concatenate([p, M.succ(p), M.pred(p), np.arange(0, 2 ** 32, 1299827, dtype=np.uint64).astype(np.uint32).view(f32),
                        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, 2.0 ** -96, 2.0 ** -97], f32)]).astype(f32)
    x.tofile(os.path.join(d, "sq_in"))
    r = subprocess.run([exe, os.path.join(d, "sq_in"), os.path.join(d, "sq_out"), "sqrt"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x.astype(f64)).astype(f32)
    assert len(x) > 4000 and np.all(bits_eq(np.fromfile(os.path.join(d, "sq_out"), f32), want))


# ---- whole programs: text == model, containment -----------------------------------------------------------------------------------
def program_boxes(p):
    """boxes for a whole program: the culler's own (a spread of the sub-boxes and coarse boxes of the 136 x 132 x 128 grid), 1-ulp and
    few-ulp boxes at grid points, boxes around the origin and the axes, wide boxes"""
    mn, mx = scene_bounds(p)
    ax, sub, coarse = culler_boxes(mn, mx, GRIDS[0])
    B = []
    for idx, step in ((sub, (5, 7, 6)), (coarse, (1, 3, 3))):
        X, Y, Z = axis_boxes(ax, idx)
        sel = [np.arange(0, len(idx[a][0]), step[a]) for a in range(3)]
        g = np.meshgrid(*sel, indexing="ij")
        B.append(np.stack([X[0].ravel()[g[0].ravel()], X[1].ravel()[g[0].ravel()], Y[0].ravel()[g[1].ravel()], Y[1].ravel()[g[1].ravel()],
                           Z[0].ravel()[g[2].ravel()], Z[1].ravel()[g[2].ravel()]], -1))
    nsub, ncoarse = len(B[0]), len(B[1])
    c = np.stack([ax[0][3:130:9][:14], ax[1][5:130:9][:14], ax[2][1:128:9][:14]], -1)
    for k in (0, 1, 3):   # degenerate, 1-ulp and 3-ulp boxes
        hi = c
        for _ in range(k):
            hi = M.succ(hi)
        B.append(np.stack([c[:, 0], hi[:, 0], c[:, 1], hi[:, 1], c[:, 2], hi[:, 2]], -1))
    z = f32(0.0)
    B.append(np.array([[-0.0, z, -0.0, z, -0.0, z], [-1, 1, -1, 1, -1, 1], [-0.25, 0.5, 0.125, 0.25, -1, -0.5], [-3, 3, -3, 3, -3, 3],
                       [-1e-3, 1e-3, 0.5, 0.75, 0.5, 0.75], [0.5, 0.75, -1e-3, 1e-3, -0.75, -0.5], [-100, 100, -1, 1, 0, 1e30],
                       [-np.inf, 1, 0, 1, 0, 1], [0, 1, 0, np.inf, -np.inf, np.inf], [np.nan, np.nan, 0, 1, 0, 1]], f32))
    return np.concatenate(B).astype(f32), nsub, ncoarse


def program_points(p, B, nsub, ncoarse):
    """the points of assertion 2: per box the culler's lattice m + (float)i * d (8 x 4 x 4, and 128 x 8 x 8 of two coarse boxes), all
    eight corners and the candidates of box_points, every float of the few-ulp boxes"""
    mn, mx = scene_bounds(p)
    ax = grid_axes(mn, mx, GRIDS[0])
    pts = []
    for i, b in enumerate(B):
        if np.isnan(b).any():
            pts.append(np.zeros((0, 3), f32))
            continue
        q = [box_points(b[None])[:, 0]]
        if i < nsub + ncoarse and (i < nsub or i % 7 == 0):
            sel = [a[(a >= b[2 * k]) & (a <= b[2 * k + 1])] for k, a in enumerate(ax)]
            assert [len(s) for s in sel] == [8, 4, 4] or i >= nsub
            g = np.meshgrid(*sel, indexing="ij")
            q.append(np.stack([x.ravel() for x in g], -1))
        fl = [all_floats(b[2 * k], b[2 * k + 1], 5) for k in range(3)]
        if all(f is not None for f in fl):
            g = np.meshgrid(*fl, indexing="ij")
            q.append(np.stack([x.ravel() for x in g], -1))
        pts.append(np.concatenate(q).astype(f32))
    return pts


def test_whole_programs_text_equals_model_and_contains_points(whole):
    """Assertions 1 and 2 for every catalogue scene, the four mathops scenes, the bound scenes, ir_interp.random_program(0..23),
    mathops_model.random_program(0..7) and the domain-safe random programs.  Known share of (program, box) pairs, from the model:
    printed below; every domain-safe program must reach a half (found: mean 0.998, least 0.992; ir_interp's random DAGs 0.653 with
    some seeds at 0, the mathops ones 0.485; every scene 0.988 to 1.0)."""
    t, exe, d = whole
    recs, meta = [], []
    for n, p in enumerate(t.programs):
        B, nsub, ncoarse = program_boxes(p)
        pts = program_points(p, B, nsub, ncoarse)
        recs.append((n, t.cuts[n][3], p["vols"], B, np.concatenate(pts)))
        meta.append((B, pts))
    res = run_host(exe, d, "whole", recs)
    known = {}
    for p, (B, pts), (iv, w) in zip(t.programs, meta, res):
        lo, hi = model_interval(p, B)
        bad = ~(bits_eq(iv[:, 0], lo) & bits_eq(iv[:, 1], hi))
        assert not bad.any(), (p["name"], "text != model", B[bad][:3], iv[bad][:3], lo[bad][:3], hi[bad][:3])
        allp = np.concatenate(pts)
        want = point_values(p, allp)
        assert np.all(bits_eq(w, want)), (p["name"], "sdf_eval of the text != the point model")
        o = 0
        for i, q in enumerate(pts):
            v = want[o:o + len(q)]
            o += len(q)
            if len(q) and not np.isnan(lo[i]):
                with np.errstate(invalid="ignore"):
                    ok = (v >= lo[i]) & (v <= hi[i])
                assert ok.all(), (p["name"], "containment", B[i], lo[i], hi[i], q[~ok][:3], v[~ok][:3])
        known[p["name"]] = float(np.mean(~np.isnan(lo[~np.isnan(B).any(axis=1)])))
    for fam in ("random_", "mrandom_", "safe_"):
        ks = [v for k, v in known.items() if k.startswith(fam)]
        print(f"known share {fam}: {np.mean(ks):.3f} (min {min(ks):.3f})")
    print("known share, scenes:", {k: round(v, 3) for k, v in known.items() if "random" not in k and "safe" not in k})
    assert np.mean([v for k, v in known.items() if k.startswith("safe_")]) >= 0.5
    assert all(v >= 0.5 for k, v in known.items() if k.startswith("safe_"))


# ---- the culler's own boxes, whole grids ------------------------------------------------------------------------------------------
REPEATS_X = ("readme_repeat_xy", "repeat_xz_box", "repeat_x_y_plain", "repeat_xy_plain")


@pytest.fixture(scope="module")
def culler_shares():
    """{(scene, dims): (share of sub-boxes decided at iso 0, share of coarse boxes decided)}: every scene, both grids, one task per
    column of coarse boxes, in a pool of processes (the numpy point model over 20 M voxels per scene is the cost)"""
    import multiprocessing
    sc = _scene_list()
    tasks = [(si, dims, x0, min(x0 + 128, dims[0])) for dims in GRIDS[::-1] for si in range(len(sc)) for x0 in range(0, dims[0], 128)]
    tasks.sort(key=lambda k: -(k[3] - k[2]) * k[1][1] * k[1][2] * len(sc[k[0]]["ops"]))
    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    with concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("fork")) as ex:
        res = list(ex.map(check_culler_chunk, tasks))
    tot = {}
    for si, dims, counts in res:
        c = tot.setdefault((sc[si]["name"], dims), {"sub": [0, 0], "coarse": [0, 0]})
        for k, (a, b) in counts.items():
            c[k][0] += a
            c[k][1] += b
    return {k: (v["sub"][0] / v["sub"][1], v["coarse"][0] / v["coarse"][1]) for k, v in tot.items()}


@pytest.mark.parametrize("dims", GRIDS)
def test_culler_boxes_contain_the_sampled_volume(culler_shares, dims):
    """Assertion 3: per sub-box, coarse box and clamped partial coarse box of the grid, the model interval contains [min, max] of the
    model's sampled volume, and a box with a NaN voxel is unknown (asserted in check_culler_chunk).  Not vacuous: on 136 x 132 x 128
    the model decides more than half of the sub-boxes of every scene at iso 0, and at least one coarse box of every scene that does
    not repeat along x (a 128-voxel box covers whole periods of RepeatX / RepeatXY; in fact the model decides coarse boxes there
    too, away from the spheres in z).
    Shares found with the model on 136 x 132 x 128 (sub-boxes / coarse boxes): sphere_w 0.978 / 0.934, box_w 0.980 / 0.934, plane_w
    0.943 / 0.732, cylinder 0.987 / 0.956, solid_sphere 0.995 / 0.974, colored_spheres 0.996 / 0.982, readme_repeat_xy 0.854 / 0.761,
    repeat_xz_box 0.897 / 0.824, repeat_x_y_plain 0.904 / 0.875, repeat_xy_plain 0.934 / 0.875, union8 0.954 / 0.877, sdf_with_color
    0.993 / 0.985, gyroid 0.818 / 0.713, twist 0.951 / 0.732, polar 0.933 / 0.882, smooth_union 0.970 / 0.930, bound_two_volumes
    0.787 / 0.500, bound_union_nearest 0.888 / 0.588, bound_union_linear 0.800 / 0.588.  On 300 x 236 x 250 the sub-box shares are
    0.855 (bound_two_volumes) to 0.998.  They are printed again by every run."""
    for p in _scene_list():
        s, c = culler_shares[(p["name"], dims)]
        print(f"{p['name']:22s} {dims}: sub-boxes decided {s:.3f}, coarse boxes decided {c:.3f}")
        if dims == GRIDS[0]:
            assert s > 0.5, (p["name"], s)
            if p["name"] not in REPEATS_X:
                assert c > 0, p["name"]


# ---- per-op edge tables -----------------------------------------------------------------------------------------------------------
def _near_multiples():
    """floats nearest to k pi / 2: every k to 64, then decades to 10^6, then every binade to FLT_MAX"""
    k = np.concatenate([np.arange(1, 65), [100, 1000, 10 ** 4, 10 ** 5, 10 ** 6, 10 ** 6 + 1]]).astype(f64)
    c = np.concatenate([(k * (np.pi / 2)).astype(f32), np.ldexp(f32(1.5707964), np.arange(21, 127)).astype(f32), [FMAX]]).astype(f32)
    return np.concatenate([c, -c])


def sincos_table():
    c = _near_multiples()
    L = [(c, c), (c, M.succ(c)), (M.pred(c), c)]
    for w in (np.nextafter(f32(4), f32(0)), f32(4), np.nextafter(f32(4), f32(8)), f32(6.4), f32(0.01), f32(1.0), f32(3.0)):
        with np.errstate(over="ignore"):
            L += [(c, np.minimum((c + w).astype(f32), FMAX)), (np.maximum((c - w).astype(f32), -FMAX), c)]
    k = np.arange(1, 9).astype(f64)
    for s in (2.0 ** -20, 2.0 ** -21, 2.0 ** -19):   # boxes ending that many quadrants short of an extremum (or a zero), and starting so
        e = ((k - s) * (np.pi / 2)).astype(f32)
        b = ((k + s) * (np.pi / 2)).astype(f32)
        L += [((e - f32(0.5)).astype(f32), e), (b, (b + f32(0.5)).astype(f32)), (-e, (-e + f32(0.5)).astype(f32))]
    L += [special_intervals(), ulp_boxes(), ivs([[0.1, 0.5], [1, 2], [0, 6.4], [-6.4, 0], [0, 5], [2, 4.5], [-1, 1], [4, 5]])]
    return cat(*L)


def _structured():
    from tests.test_mathops_codegen import structured
    v = structured()
    return np.unique(v[~np.isnan(v)])


def unary_table(extra=()):
    v = _structured()
    with np.errstate(over="ignore", invalid="ignore"):
        L = [(v, v), (v, M.succ(v)), (M.pred(v), v), (v, np.where(np.isfinite(v), (v + f32(1)).astype(f32), v)), special_intervals(), ulp_boxes()]
    return cat(*L, *extra)


def floor_table():
    k = np.array([-3, -2, -1, 0, 1, 2, 3, 7, 2.0 ** 23, -2.0 ** 23, 2.0 ** 23 - 1, 2.0 ** 23 - 0.5, -2.0 ** 23 + 0.5, 2.0 ** 24, 2.0 ** 31, -2.0 ** 31], f32)
    return cat((k, k), (M.pred(k), k), (k, M.succ(k)), (M.pred(k), M.succ(k)), ((k - f32(0.5)).astype(f32), (k + f32(0.5)).astype(f32)),
               special_intervals(), ulp_boxes())


def binary_table():
    """all pairs of the special intervals -- [finite, finite] * [x, inf], the overflow [1e30, 2e30] * [1e30, 2e30], boxes through zero
    on either side, 0 * inf inside boxes with finite corners -- and the 1-ulp boxes against a few partners"""
    a, b = cross(special_intervals(), special_intervals())
    partners = ivs([[1, 2], [-3, -1], [0.0, 0.0], [-0.0, 0.0], [-1, 1], [1e30, 2e30], [np.inf, np.inf], [-np.inf, 1]])
    u, q = cross(ulp_boxes(), partners)
    return cat(a, u, q), cat(b, q, u)


def sel_table():
    L = ivs([[1, 2], [2, 3], [2, 2], [3, 4], [-0.0, -0.0], [0.0, 0.0], [-0.0, 0.0], [-1, 0.0], [-1, -0.0], [0.0, 1], [-np.inf, np.inf],
             [np.inf, np.inf], [-np.inf, -np.inf], [1, np.inf], [np.nan, np.nan], [1, 1], [1, 3], [1.5, 2.5]])
    a, b = cross(L, L)    # a.hi == b.lo and a.lo == b.hi among them
    c = ivs([[5, 6], [8, 9], [np.nan, np.nan], [7, 7]])
    n, m = len(a[0]), len(c[0])
    rep = lambda v: (np.repeat(v[0], m), np.repeat(v[1], m))
    return rep(a), rep(b), (np.tile(c[0], n), np.tile(c[1], n))


def atan2_table():
    y = ivs([[0.0, 1], [-0.0, 1], [-1, -0.0], [-1, 0.0], [-1, 1], [1e-45, 1], [-1, -1e-45], [0.0, 0.0], [-0.0, -0.0], [-0.0, 0.0], [1, np.inf],
             [-np.inf, -1], [-np.inf, np.inf], [2, 3], [-3, -2], [np.inf, np.inf], [1e-45, 1e-45], [-1e-45, 0.0], [np.nan, np.nan]])
    x = ivs([[-2, -1], [-1, -0.0], [-1, 0.0], [-0.0, 1], [0.0, 1], [-1, 1], [1, 2], [-np.inf, -1], [1, np.inf], [-np.inf, np.inf], [0.0, 0.0],
             [-0.0, -0.0], [-0.0, 0.0], [1e-45, 1], [-1, -1e-45], [-np.inf, -np.inf], [np.inf, np.inf], [-1e-45, -1e-45], [1e30, FMAX]])
    yy, xx = cross(y, x)
    u = ulp_boxes()
    one = (np.ones(len(u[0]), f32), np.full(len(u[0]), 2, f32))
    return cat(yy, u, one), cat(xx, one, u)


def vox_table(vol, op):
    """boxes inside one cell, spanning 2, 3, 2^k and 2^k + 1 cells per axis, at the lower and the upper (ragged) end, outside the
    volume on each side, with an infinite end, degenerate"""
    n = vol[0].shape
    d, mn = VM.vol_d(vol), np.asarray(vol[2], f32)
    org = mn if op == VM.NEAREST else (mn + f32(0.5) * d).astype(f32)   # cell edges / cell centres: where the index maps step
    rows = []
    for span in (1, 2, 3, 4, 5, 8, 9, 16, 17):
        for where in (0, 1, 2, 3):   # the lower end, one cell in, the upper end, one cell short of the upper end
            for f0, f1 in ((0.25, 0.75), (0.0, 1.0), (0.0, 0.0)):
                r = []
                for a in range(3):
                    s = min(span, n[a])
                    st = (0, min(1, n[a] - s), n[a] - s, max(n[a] - s - 1, 0))[where]
                    r += [org[a] + f32(st + f0) * d[a], org[a] + f32(st + s - 1 + f1) * d[a]]
                rows.append(r)
    mxs = np.asarray(vol[3], f32)
    full = [v for a in range(3) for v in (mn[a], mn[a] + f32(1.5) * d[a])]   # (the other axes: the first two cells)
    for a in range(3):
        for lo, hi in ((mn[a] - 2 * d[a], mn[a] - d[a]), (mxs[a] + d[a], mxs[a] + 2 * d[a]), (-np.inf, mn[a]), (mxs[a], np.inf),
                       (mn[a] - d[a], mn[a] + d[a] * f32(0.5)), (-np.inf, np.inf), (np.nan, np.nan), (-FMAX, FMAX)):
            r = list(full)
            r[2 * a], r[2 * a + 1] = lo, hi
            rows.append(r)
    return np.asarray(rows, f32)


def interior_table(vol, op):
    """small boxes (1 to 4 cells per axis) on a lattice inside POISONED_VOL, away from its corners: the non-finite corner voxels
    poison the first and the last cell of every level, so most boxes of vox_table are unknown there; these are known"""
    d, mn = VM.vol_d(vol), np.asarray(vol[2], f32)
    org = mn if op == VM.NEAREST else (mn + f32(0.5) * d).astype(f32)
    rows = []
    for span in (1, 2, 3, 4):
        for x in (9, 22, 35, 50):
            for y, z in ((5, 5), (14, 9), (25, 12)):
                for f0, f1 in ((0.25, 0.75), (0.0, 1.0), (0.0, 0.0)):
                    r = []
                    for a, st in enumerate((x, y, z)):
                        r += [org[a] + f32(st + f0) * d[a], org[a] + f32(st + span - 1 + f1) * d[a]]
                    rows.append(r)
    return np.asarray(rows, f32)


def big_table(vol, op):
    """a handful of boxes for BIG_VOL: the whole volume (the top level), its upper half in x, boxes of 2, 3 and 5 cells in the second
    step of the base kernel's grid stride (x >= 164) and at the lower corner, a box on each non-finite voxel"""
    n = vol[0].shape
    d, mn = VM.vol_d(vol), np.asarray(vol[2], f32)
    org = mn if op == VM.NEAREST else (mn + f32(0.5) * d).astype(f32)
    rows = []
    for st, span in (((0, 0, 0), n), ((88, 0, 0), (88, 160, 160)), ((165, 3, 7), (2, 2, 2)), ((171, 150, 155), (3, 3, 3)), ((168, 70, 90), (5, 5, 5)),
                     ((1, 2, 1), (3, 2, 3)), ((8, 0, 0), (80, 128, 128)), ((164, 128, 128), (12, 32, 32)), ((169, 99, 32), (3, 3, 3)), ((4, 149, 149), (2, 2, 2)), ((175, 159, 159), (1, 1, 1))):
        r = []
        for a in range(3):
            r += [org[a] + f32(st[a] + 0.25) * d[a], org[a] + f32(st[a] + span[a] - 1 + 0.75) * d[a]]
        rows.append(r)
    return np.asarray(rows, f32)


def one_sided_intervals():
    lo, hi = special_intervals()
    k = (lo > 0) | (hi < 0)
    return lo[k], hi[k]


def non_negative_intervals():
    lo, hi = special_intervals()
    v = _structured()
    v = v[(v > 0) & np.isfinite(v)]
    with np.errstate(over="ignore"):
        return cat((lo[lo >= 0], hi[lo >= 0]), (v, np.minimum((v * f32(2)).astype(f32), FMAX)))


def edge_tables():
    """{program name: boxes [n, 6]}"""
    T = {}
    bx, by = binary_table()
    for k in ("add", "sub", "mul", "min_sel", "max_sel", "min_ieee", "max_ieee"):
        T["op_" + k] = boxes6(bx, by)
    da, db = cross(special_intervals(), one_sided_intervals())   # divisors on one side of zero, so that half of the table is known
    T["op_div"] = boxes6(cat(bx, da), cat(by, db))
    un = unary_table()
    for k in ("neg", "abs", "sqr", "exp", "const"):
        T["op_" + k] = boxes6(un)
    T["op_sqrt"] = T["op_log"] = boxes6(unary_table((non_negative_intervals(),)))   # (likewise: operands that do not reach below zero)
    T["op_floor"] = boxes6(floor_table())
    T["op_sin"] = T["op_cos"] = boxes6(sincos_table())
    T["op_sel_lt"] = boxes6(*sel_table())
    T["op_atan2"] = boxes6(*atan2_table())
    for vi, vol in enumerate(EDGE_VOLS):
        for nm, op in (("nearest", VM.NEAREST), ("linear", VM.LINEAR)):
            for ch in ((3, 1) if vol[1] is not None else (3,)):
                T[f"op_vox_{nm}_{vi}_{ch}"] = (big_table(vol, op) if vi == BIG_VOL else vox_table(vol, op) if vi != POISONED_VOL else
                                               np.concatenate([vox_table(vol, op), interior_table(vol, op)]))
    return T


def edge_points(name, B):
    """[k, n, 3] points inside the boxes: candidates per axis (ends, inner neighbours, midpoint, both zeros, evenly spaced ones)"""
    dense = 31 if name in ("op_sin", "op_cos") else (9 if "vox" in name else 0)
    return box_points(B, dense)


class Edge:
    """a table's model intervals and the point values inside its boxes, computed once (they do not depend on the text)"""

    def __init__(self, p, B):
        self.p, self.B = p, B
        self.lo, self.hi = model_interval(p, B)
        self.v = point_values(p, edge_points(p["name"], B))   # [k, n]
        # few-ulp boxes: every float inside (the product of the axes)
        self.extra = {}
        w = np.stack([M_ord(B[:, 2 * k + 1]) - M_ord(B[:, 2 * k]) for k in range(3)])
        few = np.isfinite(B).all(axis=1) & (w < 6).all(axis=0) & (w.max(axis=0) > 0)
        for i in np.flatnonzero(few):
            g = np.meshgrid(*[all_floats(B[i, 2 * k], B[i, 2 * k + 1], 6) for k in range(3)], indexing="ij")
            self.extra[int(i)] = point_values(p, np.stack([x.ravel() for x in g], -1))

    def judge(self, iv, sel=None):
        """(text == model, contained), per box of `sel` (all boxes by default)"""
        sel = np.arange(len(self.B)) if sel is None else sel
        same = bits_eq(iv[sel, 0], self.lo[sel]) & bits_eq(iv[sel, 1], self.hi[sel])
        ok = contained(self.v[:, sel], iv[sel, 0], iv[sel, 1])
        for n, i in enumerate(sel):
            if int(i) in self.extra and not np.isnan(iv[i, 0]):
                w = self.extra[int(i)]
                with np.errstate(invalid="ignore"):
                    ok[n] &= bool(np.all((w >= iv[i, 0]) & (w <= iv[i, 1])))
        return same, ok


def run_edge(t, exe, d, tag, tables):
    recs = [(n, t.cuts[n][3], p["vols"], tables[p["name"]], np.zeros((0, 3), f32)) for n, p in enumerate(t.programs)]
    return [r[0] for r in run_host(exe, d, tag, recs)]


@pytest.fixture(scope="module")
def edge(single):
    t, exe, d = single
    tables = edge_tables()
    return tables, [Edge(p, tables[p["name"]]) for p in t.programs], run_edge(t, exe, d, "edge", tables)


def test_edge_tables_text_equals_model_and_contains_points(single, edge):
    """Assertions 1, 2 and 4 on the per-opcode tables.  Not vacuous: at least half of every table's boxes have a known model interval
    (op_div, op_sqrt and op_log carry extra boxes with one-sided divisors / non-negative operands for that).  Found with the model:
    op_div 0.625, op_sqrt and op_log 0.552, op_mul 0.863, op_sel_lt 0.841, the volume tables 0.61 to 0.97, every other table 0.98 to
    1.0.  The shares are printed by every run."""
    t = single[0]
    _, edges, res = edge
    for p, e, iv in zip(t.programs, edges, res):
        B = e.B
        same, ok = e.judge(iv)
        assert same.all(), (p["name"], "text != model", B[~same][:4], iv[~same][:4], e.lo[~same][:4], e.hi[~same][:4])
        assert ok.all(), (p["name"], "containment", B[~ok][:4], iv[~ok][:4])
        share = float(np.mean(~np.isnan(e.lo)))
        print(f"{p['name']:22s} {len(B):6d} boxes, known {share:.3f}")
        assert share >= 0.5, (p["name"], share)


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
def _sub(old, new, count=1, within=None):
    """replace `old` by `new` (exactly `count` occurrences), inside the function whose text starts with `within`"""
    def f(t):
        a = t.index(within) if within else 0
        b = t.index("\n}\n", a) if within else len(t)
        seg = t[a:b]
        assert seg.count(old) == count, (old, seg.count(old))
        return t[:a] + seg.replace(old, new) + t[b:]
    return f


def _drop_line(marker, within):
    def f(t):
        a = t.index(within)
        i = t.index(marker, a)
        return t[:t.rindex("\n", 0, i)] + t[t.index("\n", i):]
    return f


# (name, mutation, must the result stay sound?)  "sound": the mutant is wider, not wrong -- it must differ from the model and still contain
MUTATIONS = [
    ("sincos_succ", _sub("sdfk_succ(fh)", "fh", within="sdfk_iv iv_sincos("), False),
    ("sincos_hmax", _sub("hmax ?", "false ?", within="sdfk_iv iv_sincos("), False),
    ("sincos_width", _sub("> 4.0", "> 6.5", within="sdfk_iv iv_sincos("), False),
    ("mul_zero_inf", _drop_line("0 * inf somewhere in the box", "sdfk_iv iv_mul("), False),
    ("div_first_line", _drop_line("the divisor may be zero", "sdfk_iv iv_div("), False),
    ("sel_never_tie", _sub("a.lo >= b.hi", "a.lo > b.hi", within="sdfk_iv iv_sel_lt("), True),
    ("sel_always_tie", _sub("a.hi < b.lo", "a.hi <= b.lo", within="sdfk_iv iv_sel_lt("), False),
    ("sqr_as_mul", lambda t: re.sub(r"iv_sqr\((i\d+)\);", r"iv_mul(\1, \1);", t), True),
    ("log_pred", _sub("sdfk_pred(sdfk_logf(a.lo))", "sdfk_logf(a.lo)", within="sdfk_iv iv_log("), False),
    ("atan2_cut", _sub("x.lo <= 0.0f", "x.lo < 0.0f", within="sdfk_iv iv_atan2("), False),
    ("vox_level", _sub("> 1", "> 2", count=3, within="sdfk_iv iv_vox_box("), False),
    ("vox_linear_upper", _sub("t + 1", "t", within="sdfk_iv iv_vox_linear("), False),
]
# `0x1p-20` -> `0.0` in iv_sincos is EQUIVALENT in its results and therefore not detectable: the slack only matters when an extremum
# lies within 2^-20 quadrants (1.5e-6 rad) outside an end of the box.  The function's exact value at that end is then within
# 1 - cos(1.5e-6) = 1.1e-12 of +-1, far inside the last half ulp below 1 (3e-8): a faithful f^ returns +-1 or its inner neighbour
# there, sdfk_succ / sdfk_pred of either reaches +-1, and the clamp to [-1, 1] gives exactly the +-1 the slack would have given.
EQUIVALENT = [("sincos_slack", _sub("0x1p-20", "0.0", count=2, within="sdfk_iv iv_sincos("))]


def test_mutations_of_the_text_are_detected(single, edge):
    """Assertion 5: each single textual mutation of the test's copy of the shipped text makes assertion 1 (text == model) or 2
    (containment) fail on the edge tables; the mutants that are sound but wide (iv_sqr as iv_mul(a, a); `a.lo > b.hi`, which only
    gives up a decision) must differ from the model and still contain every point.  (Only the boxes whose interval differs from
    the shipped text's are judged again: the others were judged with the shipped text.)"""
    t, _, d = single
    tables, edges, shipped = edge
    todo = MUTATIONS + [(n, f, None) for n, f in EQUIVALENT]

    def one(m):
        exe = t.build(d, m[0], m[1])
        return run_edge(t, exe, d, m[0], tables)
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        results = list(ex.map(one, todo))
    for (name, _, sound), res in zip(todo, results):
        differs, unsound = [], []
        for p, e, iv, iv0 in zip(t.programs, edges, res, shipped):
            sel = np.flatnonzero(~(bits_eq(iv[:, 0], iv0[:, 0]) & bits_eq(iv[:, 1], iv0[:, 1])))
            if len(sel) == 0:
                continue
            same, ok = e.judge(iv, sel)
            if not same.all():
                differs.append((p["name"], int((~same).sum())))
            if not ok.all():
                unsound.append((p["name"], int((~ok).sum())))
        print(f"{name:18s} text != model: {differs}   containment fails: {unsound}")
        if sound is None:
            assert not differs and not unsound, (name, "documented as equivalent")
        else:
            assert differs or unsound, (name, "NOT detected")
            if sound:
                assert differs and not unsound, name
