"""MathF.Sin / Cos / Exp / Log / Atan2 in GPU SDF programs (SDFK_OP_SIN .. SDFK_OP_ATAN2) on the MI355X: the arithmetic the JIT pastes
walked over every float (sin, cos, exp, log) and over 2^26 structured pairs (atan2) against the device's binary64 library rounded
once; SdfEx.Sample, the sampler with colours, meshes (stored = the oracle's marching of the model volume, elided and culled = stored),
the ray marcher, all bit for bit against the numpy model (tests/mathops_model.py) on four scenes -- a gyroid, a twist, a polar repeat
and an exp/log smooth union; random programs that mix the new ops into the IR; and the node path."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from sdfkit_amd import _native as N
from sdfkit_amd.api import Mesh, Sdf
from sdfkit_amd.expr import MathF, Mod, Vec3, Vec4, trace
from tests import mathops_model as M
from tests.test_gpu_parity import assert_mesh_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
TWO_PI = 6.2831855


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- four scenes -----------------------------------------------------------------------------------------------------------------
def gyroid(p):
    """a gyroid sheet cut by a sphere; colours from sin / exp"""
    s = 4.0
    x, y, z = p.x * s, p.y * s, p.z * s
    g = (MathF.Sin(x) * MathF.Cos(y) + MathF.Sin(y) * MathF.Cos(z)) + MathF.Sin(z) * MathF.Cos(x)
    w = MathF.Max(abs(g) / s - 0.08, p.Length() - 1.2)
    return Vec4.of(Vec3(0.5 + 0.5 * MathF.Sin(x), 0.5 + 0.5 * MathF.Cos(y), MathF.Exp(-p.Length())), w)


def twist(p):
    """SdfExprEx.ModifyInput rotating p about y by an angle proportional to p.Y, then a box"""
    a = p.y * 2.0
    c, s = MathF.Cos(a), MathF.Sin(a)
    q = Vec3(c * p.x - s * p.z, p.y, s * p.x + c * p.z)
    d = Vec3.Abs(q) - Vec3(p.x.b.const(0.5), p.x.b.const(0.9), p.x.b.const(0.3))
    outside = Vec3.Max(d, 0.0).Length()
    inside = MathF.Min(MathF.Max(d.x, MathF.Max(d.y, d.z)), 0.0)
    return Vec4.of(Vec3(MathF.Atan2(q.z, q.x) / 3.1415927, c, s), outside + inside)


def polar(p):
    """a polar repeat: six spheres around y, sector from MathF.Atan2"""
    n = 6.0
    sector = TWO_PI / n
    a = MathF.Atan2(p.z, p.x)
    k = Mod(a + sector * 0.5, sector) - sector * 0.5
    r = MathF.Sqrt(p.x * p.x + p.z * p.z)
    q = Vec3(r * MathF.Cos(k) - 0.8, p.y, r * MathF.Sin(k))
    return Vec4.of(Vec3(MathF.Cos(a), MathF.Sin(a), a), q.Length() - 0.3)


def smooth_union(p):
    """exponential smooth union of two spheres: -log(exp(-k a) + exp(-k b)) / k"""
    kk = 8.0
    a = (p - Vec3(p.x.b.const(-0.4), p.x.b.const(0.0), p.x.b.const(0.0))).Length() - 0.5
    b = (p - Vec3(p.x.b.const(0.45), p.x.b.const(0.1), p.x.b.const(0.0))).Length() - 0.4
    w = -MathF.Log(MathF.Exp(a * -kk) + MathF.Exp(b * -kk)) / kk
    return Vec4.of(Vec3(MathF.Exp(a), MathF.Log(abs(b) + 1e-3), MathF.Exp(p.y)), w)


SCENES = {"gyroid": gyroid, "twist": twist, "polar": polar, "smooth_union": smooth_union}
BOX = ([-1.5, -1.5, -1.5], [1.5, 1.5, 1.5])


@pytest.fixture(scope="module")
def scenes(gpu):
    return {k: (Sdf(fn, True), *trace(fn, True)) for k, fn in SCENES.items()}


# ---- the arithmetic, walked ----------------------------------------------------------------------------------------------------
HARNESS = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
@MATH@
__device__ __forceinline__ long long ord32(float v) { const int i = __builtin_bit_cast(int, v); return i < 0 ? -(long long)(i & 0x7fffffff) : i; }
__device__ __forceinline__ int dist(float g, float w) { if (g != g || w != w) return (g != g && w != w) ? 0 : 2; const long long d = ord32(g) - ord32(w); return d == 0 ? 0 : (d == 1 || d == -1 ? 1 : 2); }
__global__ void walk(int fn, unsigned long long* cnt)
{
    unsigned long long far = 0, ncr = 0;
    for (uint64_t b = blockIdx.x * 256ull + threadIdx.x; b < (1ull << 32); b += gridDim.x * 256ull) {
        const float x = __builtin_bit_cast(float, (uint32_t)b);
        float g, w;
        if (fn == 0) { g = sdfk_sinf(x); w = (float)sin((double)x); }
        else if (fn == 1) { g = sdfk_cosf(x); w = (float)cos((double)x); }
        else if (fn == 2) { g = sdfk_expf(x); w = (float)exp((double)x); }
        else { g = sdfk_logf(x); w = (float)log((double)x); }
        const int d = dist(g, w);
        far += d > 1; ncr += d == 1;
    }
    atomicAdd(cnt, far); atomicAdd(cnt + 1, ncr);
}
__device__ float pick(uint32_t h, int mode)
{
    const float r = __builtin_bit_cast(float, h & 0x7f7fffffu);   // finite, any exponent
    const float s = (h & 0x80000000u) ? -1.0f : 1.0f;
    switch (mode) { case 0: return s * 0.0f; case 1: return s * __builtin_inff(); default: return s * r; }
}
__global__ void walk2(unsigned long long* cnt)
{
    unsigned long long far = 0, ncr = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < (1u << 26); i += gridDim.x * 256u) {
        uint32_t h = i * 2654435761u ^ (i >> 7) * 40503u, h2 = h * 2246822519u + 374761393u;
        const int kind = i & 15;
        float y = pick(h, 2), x = pick(h2, 2);
        if (kind == 0) y = pick(h, 0);                                   // signed zeros
        else if (kind == 1) x = pick(h2, 0);
        else if (kind == 2) { y = pick(h, 0); x = pick(h2, 0); }
        else if (kind == 3) y = pick(h, 1);                              // infinities
        else if (kind == 4) x = pick(h2, 1);
        else if (kind == 5) { y = pick(h, 1); x = pick(h2, 1); }
        else if (kind <= 9) x = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, y) + (int)(h2 % 64) - 32) * ((h2 & 64) ? -1.0f : 1.0f);   // ratios near +-1
        else if (kind <= 11) x = y * __builtin_ldexpf(1.0f, (int)(h2 % 60) + 1) * ((h2 & 64) ? -1.0f : 1.0f);   // ratios near 0
        else if (kind == 12) y = x * __builtin_ldexpf(1.0f, (int)(h2 % 60) + 1);                               // near +-inf
        else if (kind == 13) { y = __builtin_ldexpf(y, -100); }
        const float g = sdfk_atan2f(y, x), w = (float)atan2((double)y, (double)x);
        const int d = dist(g, w);
        far += d > 1; ncr += d == 1;
    }
    atomicAdd(cnt, far); atomicAdd(cnt + 1, ncr);
}
int main(int argc, char** argv)
{
    unsigned long long* cnt;
    if (hipMalloc(&cnt, 16) != hipSuccess) return 2;
    int bad = 0;
    for (int fn = 0; fn < 5; fn++) {
        if (hipMemset(cnt, 0, 16) != hipSuccess) return 2;
        if (fn < 4) hipLaunchKernelGGL(walk, dim3(256 * 64), dim3(256), 0, 0, fn, cnt);
        else hipLaunchKernelGGL(walk2, dim3(256 * 16), dim3(256), 0, 0, cnt);
        if (hipDeviceSynchronize() != hipSuccess) return 3;
        unsigned long long h[2];
        if (hipMemcpy(h, cnt, 16, hipMemcpyDeviceToHost) != hipSuccess) return 3;
        printf("fn %d far %llu not_cr %llu\n", fn, h[0], h[1]);
        bad |= h[0] != 0;
    }
    return bad;
}
"""


def test_every_float_within_one_ulp(scenes, tmp_path):
    """sin, cos, exp, log over all 2^32 floats and atan2 over 2^26 structured pairs: 0 results more than 1 ulp from the device's
    binary64 functions rounded once; the ones that differ by 1 ulp are printed (the reference is itself rounded twice)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    sdf = scenes["gyroid"][0]
    L = N.lib()
    L.sdfk_program_source.restype = C.c_char_p
    src = L.sdfk_program_source(sdf.program()).decode()
    m = re.search(r"(#define SDFK_M_FN .*?)\n// ---- interval forms of the five", src, re.S)
    assert m, "math prelude not found in the generated source"
    (tmp_path / "walk.hip").write_text(HARNESS.replace("@MATH@", m.group(1)))
    exe = tmp_path / "walk"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", str(tmp_path / "walk.hip"), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    r = subprocess.run(["timeout", "-k", "10", "600", str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.count(" far 0 ") == 5, r.stdout + r.stderr
    shutil.rmtree(tmp_path, ignore_errors=True)


# ---- programs -----------------------------------------------------------------------------------------------------------------
def test_eval_points_matches_model(scenes):
    rng = np.random.default_rng(3)
    n = 1_000_000
    pts = rng.uniform(-3, 3, (n, 3)).astype(f32)
    bits = rng.integers(0, 2 ** 32, (n // 10, 3), dtype=np.uint64).astype(np.uint32).view(f32)
    pts[: n // 10] = bits                                   # every exponent, NaN and inf included
    pts[n // 10: n // 10 + 8] = [[0, 0, 0], [-0.0, -0.0, -0.0], [np.inf, 0, 0], [-np.inf, 1, 0], [np.nan, 0, 0], [0, np.nan, 1],
                                 [3e38, -3e38, 1e-45], [-1e-45, 88.8, -104]]
    for name, (sdf, ops, out) in scenes.items():
        got = sdf.Sample(pts)
        want = M.run(ops, out, pts)
        for k in range(4):
            assert _eq(got[:, k], want[k]), (name, k)


@pytest.mark.parametrize("dims", [(37, 29, 33), (64, 48, 256), (17, 40, 9)])
def test_sampler_matches_model(scenes, dims):
    for name, (sdf, ops, out) in scenes.items():
        for clip in (False, True):
            got = sdf.ToVoxels(*BOX, *dims, clipToBounds=clip)
            wv, wc = M.sample(ops, out, True, *BOX, *dims, clip=clip)
            assert _eq(got.Values, wv), (name, clip)
            assert _eq(got.Colors, wc), (name, clip)


@pytest.mark.parametrize("dims", [(96, 80, 72), (264, 260, 256)])
def test_meshes_stored_is_the_oracles_and_default_is_stored(scenes, dims):
    for name, (sdf, ops, out) in scenes.items():
        if dims[0] > 200 and name != "gyroid":
            continue
        mv, mc = M.sample(ops, out, True, *BOX, *dims, clip=True)
        om = O.march(mv, mc, *BOX)
        assert len(om.vertices) > 500, name
        with N.option(N.OPT_ELIDE_VOLUME, 0):
            stored = sdf.ToMesh(*BOX, *dims)
        assert_mesh_equal(stored, om)
        for mode in (2, 1):
            with N.option(N.OPT_ELIDE_VOLUME, mode):
                m = sdf.ToMesh(*BOX, *dims)
            assert np.array_equal(m.Triangles, stored.Triangles), (name, mode)
            assert _eq(m.Vertices, stored.Vertices) and _eq(m.Colors, stored.Colors), (name, mode)
        m = sdf.ToMesh(*BOX, *dims)   # (the product default)
        assert np.array_equal(m.Triangles, stored.Triangles) and _eq(m.Vertices, stored.Vertices), name


def test_raymarch_matches_model(scenes):
    w, h = 64, 40
    cam, vpi = O.ray_camera(O.look_at((0.5, 1.0, 4.0), (0, 0, 0), (0, 1, 0)), 60.0, w, h, 1.0, 100.0)
    for name, (sdf, ops, out) in scenes.items():
        depth, rgb = np.empty((h, w), f32), np.empty((h, w, 3), f32)
        N.check(N.lib().sdfk_raymarch(sdf.program(), w, h, N.f3(np.asarray(cam, f32).reshape(-1)),
                                      (C.c_float * 16)(*np.asarray(vpi, f32).reshape(-1)), C.c_float(1.0), C.c_float(100.0), 48,
                                      depth.ctypes.data, rgb.ctypes.data))
        md, mrgb = M.raymarch(ops, out, True, (), w, h, cam, vpi, 1.0, 100.0, 48)
        assert _eq(depth, md), name
        assert _eq(rgb, mrgb), name
        assert np.sum(depth < 10) > 50, name


@pytest.mark.parametrize("seed", range(8))
def test_random_programs_elided_equals_stored(gpu, seed):
    ops, out = M.random_program(seed)
    arr = (N.Op * len(ops))()
    for i, (op, a, b, c, d, imm) in enumerate(ops):
        arr[i].opcode, arr[i].a, arr[i].b, arr[i].c, arr[i].d, arr[i].imm = op, a, b, c, d, imm
    prog = C.c_void_p()
    N.check(N.lib().sdfk_program_create(arr, len(ops), (C.c_int32 * 4)(*out), 1, C.byref(prog)))
    try:
        mn, mx, dims = (-2.5, -2.0, -2.25), (2.25, 2.5, 2.0), (136, 132, 128)
        meshes = {}
        for mode in (0, 2, 1):
            with N.option(N.OPT_ELIDE_VOLUME, mode):
                for clip in (1, 0):
                    h = C.c_void_p()
                    N.check(N.lib().sdfk_sample_march(prog, N.f3(mn), N.f3(mx), *dims, clip, C.c_float(0.0), 1, C.byref(h)))
                    meshes[(mode, clip)] = Mesh._from_handle(h)
        for clip in (1, 0):
            s = meshes[(0, clip)]
            for mode in (2, 1):
                m = meshes[(mode, clip)]
                assert np.array_equal(m.Triangles, s.Triangles), (mode, clip)
                assert _eq(m.Vertices, s.Vertices) and _eq(m.Colors, s.Colors), (mode, clip)
        vol = C.c_void_p()
        small = (23, 19, 21)
        N.check(N.lib().sdfk_volume_create(*small, N.f3(mn), N.f3(mx), 1, C.byref(vol)))
        try:
            N.check(N.lib().sdfk_sample(prog, vol, 0))
            gv, gc = np.empty(small, f32), np.empty(small + (3,), f32)
            N.check(N.lib().sdfk_volume_download(vol, gv.ctypes.data, gc.ctypes.data))
        finally:
            N.lib().sdfk_volume_free(vol)
        wv, wc = M.sample(ops, out, True, mn, mx, *small)
        assert _eq(gv, wv) and _eq(gc, wc)
    finally:
        N.lib().sdfk_program_destroy(prog)


def test_node_world_one_equals_one_gpu(scenes):
    from sdfkit_amd import dist as D
    sdf = scenes["gyroid"][0]
    n = 96
    one = sdf.ToMesh(*BOX, n, n, n)
    with D.Node([0]) as node:
        m = node.to_mesh(sdf, *BOX, n, n, n)
    assert len(one.Vertices) > 1000
    assert np.array_equal(m.Triangles, one.Triangles)
    assert _eq(m.Vertices, one.Vertices) and _eq(m.Colors, one.Colors)
