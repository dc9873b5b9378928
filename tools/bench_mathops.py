"""MathF.Sin / Cos / Exp / Log / Atan2 in SDF programs (SDFK_OP_SIN .. SDFK_OP_ATAN2) on the MI355X: one JSON line.

  The scene: a gyroid sheet (six sin / cos per point) cut by a sphere, colours from sin, cos and exp (tests/test_gpu_mathops.py).
  compile:  first-call hiprtc time of a new structure (the sampler module and the block-culling pair), code-object cache off
  sample:   the gyroid sampled into a 512^3 colour volume (Voxels.SampleSdf, 16 B per voxel stored); for comparison the one-
            primitive colour sampler (SdfExprs.Sphere(1, colour)) into the same volume
  mesh:     ToMesh at 512^3, stored volume (SDFK_OPT_ELIDE_VOLUME = 0) and product default (2: elided, block culling)
  image:    one 1920 x 1080 RayMarcher frame (depth + colour) with 256 depth iterations
  points:   10^6 uniform points through SdfEx.Sample
Times are host wall clock around work that ends in a device synchronise (median of --reps, min and max as the spread).
Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script.
  python tools/bench_mathops.py [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

f32 = np.float32


def _times(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def gyroid(p):
    from sdfkit_amd.expr import MathF, Vec3, Vec4
    s = 4.0
    x, y, z = p.x * s, p.y * s, p.z * s
    g = (MathF.Sin(x) * MathF.Cos(y) + MathF.Sin(y) * MathF.Cos(z)) + MathF.Sin(z) * MathF.Cos(x)
    w = MathF.Max(abs(g) / s - 0.08, p.Length() - 1.2)
    return Vec4.of(Vec3(0.5 + 0.5 * MathF.Sin(x), 0.5 + 0.5 * MathF.Cos(y), MathF.Exp(-p.Length())), w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from sdfkit_amd.api import Sdf
    N.init()
    L = N.lib()
    sync = lambda: L.sdfk_synchronize()  # noqa: E731
    out = {}
    box = [-1.5] * 3, [1.5] * 3

    # 0. first call of a new structure: hiprtc, with the on-disk cache off
    with N.option(N.OPT_CODE_CACHE, 0):
        sdf = Sdf(gyroid, True)
        dst = K.Voxels(*box, 64, 64, 64)
        dh = dst._ensure_device(True)
        t0 = time.perf_counter()
        N.check(L.sdfk_sample(sdf.program(), dh, 0))
        sync()
        out["first_sample_compile_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        sdf.ToMesh(*box, 256, 256, 256)
        sync()
        out["first_tomesh_256_compile_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        del dst

    # 1. the sampler, 512^3 with colours
    dst = K.Voxels(*box, 512, 512, 512)
    dh = dst._ensure_device(True)
    prog = sdf.program()
    out["sample_512_gyroid_color"] = _times(lambda: N.check(L.sdfk_sample(prog, dh, 0)), args.reps, sync)
    sphere = K.SdfExprs.Sphere(1.0, (0.25, 0.5, 0.75)).ToSdf()   # (kept alive: the Sdf owns its program)
    sp = sphere.program()
    out["sample_512_sphere_color"] = _times(lambda: N.check(L.sdfk_sample(sp, dh, 0)), args.reps, sync)
    out["sample_gyroid_over_sphere"] = round(out["sample_512_gyroid_color"]["median_ms"] / out["sample_512_sphere_color"]["median_ms"], 2)
    out["gyroid_gvoxels_per_s"] = round(512 ** 3 / (out["sample_512_gyroid_color"]["median_ms"] * 1e-3) / 1e9, 1)
    del dst

    # 2. ToMesh at 512^3
    for mode, name in ((0, "stored"), (2, "default")):
        with N.option(N.OPT_ELIDE_VOLUME, mode):
            out[f"tomesh_512_{name}"] = _times(lambda: sdf.ToMesh(*box, 512, 512, 512).Vertices, args.reps, sync)
    out["tomesh_512_vertices"] = len(sdf.ToMesh(*box, 512, 512, 512).Vertices)

    # 3. one 1920 x 1080 frame, 256 iterations
    rm = K.RayMarcher(1920, 1080, sdf)
    rm.DepthIterations = 256
    out["raymarch_1920x1080x256"] = _times(lambda: rm.Render(), args.reps, sync)

    # 4. 10^6 points
    rng = np.random.default_rng(0)
    Q = rng.uniform(-1.5, 1.5, (1_000_000, 3)).astype(f32)
    res = np.zeros((len(Q), 4), f32)
    out["eval_points_1e6"] = _times(lambda: sdf.Sample(Q, res), args.reps, sync)
    n, hits, ms = C.c_int64(), C.c_int64(), C.c_double()
    L.sdfk_jit_stats(C.byref(n), C.byref(hits), C.byref(ms))
    out["jit_compiled"], out["jit_compile_ms_total"] = n.value, round(ms.value, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
