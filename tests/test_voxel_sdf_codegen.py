"""CPU checks of programs that read voxel volumes (SDFK_OP_VOXEL_NEAREST / SDFK_OP_VOXEL_LINEAR): the code generator built as host
C++ (tests/cpp/codegen_host.cpp) leaves the source of every volume-less program byte for byte as it was (SHA-256s recorded before
volumes existed, tests/golden/codegen_sha256.json: the output of this file's `codegen` fixture run on the tree before the volume
opcodes, hashed); bound programs compile for gfx950 offline (sdfk_program_check_bound); bad
slots, channels and volume counts are refused; the numpy model's nearest read is the reference's indexer, and its pyramid bound
contains every value the point forms produce."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import ir_interp as I
from sdfkit_amd import _native as N
from sdfkit_amd import Voxels
from sdfkit_amd.expr import trace
from tests import scenes
from tests import voxel_sdf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
X, Y, Z = (1, -1, -1, -1, -1, 0.0), (2, -1, -1, -1, -1, 0.0), (3, -1, -1, -1, -1, 0.0)


@pytest.fixture(scope="module")
def codegen(tmp_path_factory):
    d = tmp_path_factory.mktemp("codegen")
    exe = str(d / "codegen_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "codegen_host.cpp"), "-o", exe])

    def run(progs):
        b = bytearray()
        for ops, out, wc, nvol in progs:
            b += struct.pack("<7i", len(ops), *out, wc, nvol)
            for (op, a, bb, c, dd, imm) in ops:
                b += struct.pack("<5if", op, a, bb, c, dd, imm)
        src, dst = str(d / "in"), str(d / "out")
        open(src, "wb").write(bytes(b))
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and "codegen ok" in p.stdout, p.stderr
        data, res, o = open(dst, "rb").read(), [], 0
        while o < len(data):
            st, n = struct.unpack_from("<2i", data, o)
            res.append((st == 1, data[o + 8:o + 8 + n].decode()))
            o += 8 + n
        return res
    return run


def _catalogue():
    progs = []
    for name, mk in scenes.CATALOGUE.items():
        _, sdf = mk()
        ops, out = trace(sdf.fn, sdf.writes_color)
        progs.append((name, ops, out, int(sdf.writes_color)))
    for seed in range(24):
        ops, out = I.random_program(seed)
        progs.append((f"random_{seed}", ops, out, 1))
    return progs


def test_volume_less_sources_are_unchanged(codegen):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "codegen_sha256.json")))
    progs = _catalogue()
    assert set(want) == {p[0] for p in progs}
    for nvol in (0, 3):   # (binding volumes a program does not read changes nothing either)
        res = codegen([(ops, out, wc, nvol) for _, ops, out, wc in progs])
        for (name, *_), (ok, src) in zip(progs, res):
            assert ok, (name, src)
            assert hashlib.sha256(src.encode()).hexdigest() == want[name], name


def _vol_prog(op=M.LINEAR, d=3):
    ops = [X, Y, Z, (op, 0, 1, 2, d, 0.0), (0, -1, -1, -1, -1, 0.25), (4, 3, 4, -1, -1, 0.0)]
    return ops, [-1, -1, -1, 5]


def test_bound_source_reads_the_table(codegen):
    ops, out = _vol_prog()
    ok, src = codegen([(ops, out, 0, 1)])[0]
    assert ok, src
    assert "struct SdfkK { float k[1]; const SdfkVol* V; };" in src
    assert "sdfk_vox_linear(K.V[0], 3, v0, v1, v2)" in src and "iv_vox_linear(K.V[0], 3, i0, i1, i2)" in src


@pytest.mark.parametrize("d,nvol,msg", [(3, 0, "none is bound"), ((1 << 2) | 3, 1, "slot 1 is not bound"), (-1, 2, "is not bound"),
                                        ((8 << 2) | 3, 8, "not bound")])
def test_codegen_refuses_bad_slots(codegen, d, nvol, msg):
    ops, out = _vol_prog(M.NEAREST, d)
    ok, err = codegen([(ops, out, 0, nvol)])[0]
    assert not ok and msg in err, err


def _arr(ops):
    a = (N.Op * len(ops))()
    for i, (op, x, y, z, w, imm) in enumerate(ops):
        a[i].opcode, a[i].a, a[i].b, a[i].c, a[i].d, a[i].imm = op, x, y, z, w, imm
    return a


def test_check_bound_compiles_for_gfx950():
    ops = [X, Y, Z, (M.NEAREST, 0, 1, 2, 3, 0.0), (M.LINEAR, 0, 1, 2, (1 << 2) | 0, 0.0), (M.LINEAR, 0, 1, 2, (1 << 2) | 1, 0.0),
           (M.LINEAR, 0, 1, 2, (1 << 2) | 2, 0.0), (0, -1, -1, -1, -1, 0.5), (4, 3, 7, -1, -1, 0.0), (14, 8, 4, -1, -1, 0.0)]
    out = (C.c_int32 * 4)(4, 5, 6, 9)
    assert N.lib().sdfk_program_check_bound(_arr(ops), len(ops), out, 1, 2) == 0, N.lib().sdfk_last_error()


def test_unbound_entry_points_refuse_volume_opcodes():
    ops, out = _vol_prog()
    o = (C.c_int32 * 4)(*out)
    assert N.lib().sdfk_program_check(_arr(ops), len(ops), o, 0) == 1
    assert b"none is bound" in N.lib().sdfk_last_error()
    assert N.lib().sdfk_program_check_bound(_arr(ops), len(ops), o, 0, 9) == 1          # more than 8 volumes
    assert N.lib().sdfk_program_check_bound(_arr(ops), len(ops), o, 0, -1) == 1
    ops, out = _vol_prog(M.NEAREST, (2 << 2) | 3)
    assert N.lib().sdfk_program_check_bound(_arr(ops), len(ops), (C.c_int32 * 4)(*out), 0, 2) == 1


def test_model_nearest_is_the_reference_indexer():
    rng = np.random.default_rng(3)
    for shape, mn, mx in [((7, 5, 9), (-1.0, -2.0, 0.5), (1.5, 2.0, 3.0)), ((1, 4, 2), (0.0, 0.0, 0.0), (1.0, 0.3, 0.7)),
                          ((16, 16, 16), (-1.1, -1.1, -1.1), (1.1, 1.1, 1.1))]:
        vals = rng.standard_normal(shape).astype(f32)
        vox = Voxels(vals, None, mn, mx)
        pts = rng.uniform(np.array(mn) - 0.3, np.array(mx) + 0.3, (600, 3)).astype(f32)
        # exact cell boundaries and centres as well
        d = M.vol_d((vals, None, mn, mx))
        k = np.stack([rng.integers(0, n, 200) for n in shape], -1)
        pts = np.concatenate([pts, (np.asarray(mn, f32) + k * d).astype(f32), (np.asarray(mn, f32) + (k + f32(0.5)) * d).astype(f32)])
        got = M.nearest((vals, None, mn, mx), 3, pts[:, 0], pts[:, 1], pts[:, 2])
        n_in = 0
        for p, g in zip(pts, got):
            ix = vox._index_of(p)
            if all(0 <= i < n for i, n in zip(ix, shape)):   # where the reference does not throw
                assert g == vals[ix], (p, ix)
                n_in += 1
        assert n_in > 300


def test_model_pyramid_bound_contains_point_values():
    rng = np.random.default_rng(5)
    shape, mn, mx = (13, 6, 21), (-1.0, -0.5, -2.0), (1.0, 0.5, 2.0)
    vals = rng.standard_normal(shape).astype(f32)
    vals[3, 2, 7] = np.inf
    vol = (vals, None, mn, mx)
    lv = M.pyramid(vals)
    for _ in range(300):
        lo = rng.uniform(np.array(mn) - 0.5, np.array(mx) + 0.5).astype(f32)
        hi = (lo + rng.uniform(0, 1.5, 3)).astype(f32)
        pts = rng.uniform(lo, hi, (64, 3)).astype(f32)
        pts = np.concatenate([pts, lo[None], hi[None]])
        for op, fn in ((M.NEAREST, M.nearest), (M.LINEAR, M.linear)):
            b = M.interval(vol, 3, op, (lo[0], hi[0]), (lo[1], hi[1]), (lo[2], hi[2]), lv)
            if np.isnan(b[0]):
                continue
            v = fn(vol, 3, pts[:, 0], pts[:, 1], pts[:, 2])
            assert np.all((v >= b[0]) & (v <= b[1])), (op, lo, hi)
