"""Voxels.Redistance (sdfk_volume_redistance, csrc/lib_redistance.hip) on the MI355X: one JSON line.

  mesh256:  the clipped 512^3 mesh of Sdfs.Sphere(1) over -1.25..1.25 (DESIGN.md 8b's case) into 256^3: MeshSdf.ToVoxels with
            a band of 4 voxels, Redistance() of it, and -- once, unless --skip-unbanded -- the only route the library had to the
            same full field before: ToVoxels unbanded.
  field512: Redistance() at 512^3 of the sphere 3 (|p| - 1), of tools/bench_mathops.py's gyroid and of a union of 8 primitives:
            ms, sweeps, tile-sweeps executed against those a full Jacobi iteration makes, bytes moved per tile-sweep.
  raymarch: 1920 x 1080, 256 iterations through vox.ToSdf() before and after Redistance(): the fraction of pixels whose depth
            differs from a 1024-iteration render of the same volume by more than one voxel.
A call synchronises with the host once per batch of queued sweeps, so times are host wall clock around the call and a final
device synchronise (median of --reps after a warm-up call; min and max are the spread).  Kernel times: a rocprofv3
--kernel-trace --stats run of this script with --trace (one repetition, no unbanded volume, no ray marching).
  python tools/bench_redistance.py [--reps 5] [--skip-unbanded] [--trace]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

f32 = np.float32
# a swept tile reads its 512 voxels and six 64-voxel faces and writes 512 voxels (f32), plus seven flag words and its own
TILE_BYTES = (512 + 6 * 64 + 512) * 4 + 8 * 4


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


def union8(p):
    from sdfkit_amd.expr import MathF, Vec3, Vec4
    w = None
    for i in range(8):
        c = Vec3(0.7 * (1 if i & 1 else -1), 0.7 * (1 if i & 2 else -1), 0.7 * (1 if i & 4 else -1))
        d = (p - c).Length() - (0.35 + 0.03 * i)
        w = d if w is None else MathF.Min(w, d)
    return Vec4.of(Vec3(1.0, 1.0, 1.0), w)


def sphere3(p):
    from sdfkit_amd.expr import Vec3, Vec4
    return Vec4.of(Vec3(1.0, 1.0, 1.0), 3.0 * (p.Length() - 1.0))


def _redistance_record(K, vox, reps, sync, band=float("inf")):
    st = {}
    rec = _times(lambda: vox.Redistance(maxDistance=band), reps, sync)
    vox.Redistance(maxDistance=band, stats=st)
    tiles = -(-vox.NX // 8) * -(-vox.NY // 8) * -(-vox.NZ // 8)
    rec.update(st)
    rec["tile_sweeps_full_jacobi"] = st["sweeps"] * tiles
    rec["active_fraction"] = round(st["tile_sweeps"] / max(st["sweeps"] * tiles, 1), 4)
    rec["bytes_per_tile_sweep"] = TILE_BYTES
    rec["tb_per_s_of_8"] = round(st["tile_sweeps"] * TILE_BYTES / (rec["median_ms"] * 1e-3) / 1e12, 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-unbanded", action="store_true")
    ap.add_argument("--trace", action="store_true", help="one repetition of the Redistance calls only (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from sdfkit_amd.api import Sdf
    from sdfkit_amd.meshsdf import MeshSdf
    from bench_mathops import gyroid
    N.init()
    L = N.lib()
    sync = lambda: L.sdfk_synchronize()  # noqa: E731
    reps = 1 if args.trace else args.reps
    out = {}

    # 1. banded mesh volume -> Redistance, against the unbanded mesh volume
    box = [-1.25] * 3, [1.25] * 3
    m = K.Sdfs.Sphere(1.0).ToMesh(*box, 512, 512, 512, clipToBounds=True)
    t = MeshSdf((np.array(m.Vertices, f32), np.array(m.Triangles, np.int32)))
    n, cell = 256, 2.5 / 256
    out["mesh256_triangles"] = len(m.Triangles) // 3
    out["mesh256_to_voxels_band_4vox"] = _times(lambda: t.ToVoxels(*box, n, n, n, maxDistance=4 * cell), reps, sync)
    banded = t.ToVoxels(*box, n, n, n, maxDistance=4 * cell)
    out["mesh256_redistance"] = _redistance_record(K, banded, reps, sync)
    out["mesh256_banded_plus_redistance_ms"] = round(out["mesh256_to_voxels_band_4vox"]["median_ms"] + out["mesh256_redistance"]["median_ms"], 3)
    if not args.skip_unbanded and not args.trace:
        t0 = time.perf_counter()
        full = t.ToVoxels(*box, n, n, n)
        sync()
        out["mesh256_to_voxels_unbanded_ms_once"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["mesh256_speedup_over_unbanded"] = round(out["mesh256_to_voxels_unbanded_ms_once"] / out["mesh256_banded_plus_redistance_ms"], 1)
        d = np.abs(banded.Redistance().Values.astype(np.float64) - full.Values.astype(np.float64)) / cell
        out["mesh256_vs_exact_voxels"] = {"max": round(float(d.max()), 4), "mean": round(float(d.mean()), 4)}
        del full

    # 2. 512^3 fields
    box = [-1.5] * 3, [1.5] * 3
    for name, fn in (("sphere3", sphere3), ("gyroid", gyroid), ("union8", union8)):
        vox = K.Voxels.SampleSdf(Sdf(fn, True), *box, 512, 512, 512)
        out[f"field512_{name}"] = _redistance_record(K, vox, reps, sync)
        del vox
    if args.trace:
        print(json.dumps(out))
        return

    # 3. what sphere tracing gains: 256 fixed iterations against 1024 on the same volume
    for name, fn in (("sphere3", sphere3), ("gyroid", gyroid)):
        vox = K.Voxels.SampleSdf(Sdf(fn, True), *box, 256, 256, 256)
        for tag, v in (("before", vox), ("after", vox.Redistance())):
            sdf = v.ToSdf()
            rm = K.RayMarcher(1920, 1080, sdf)
            rm.DepthIterations = 256
            d256 = np.array(rm.RenderDepth().Values, f32)
            rm.DepthIterations = 1024
            d1024 = np.array(rm.RenderDepth().Values, f32)
            both = np.isfinite(d256) & np.isfinite(d1024)
            out[f"raymarch_{name}_{tag}_fraction_off_by_a_voxel"] = round(float(np.mean(~both | (np.abs(d256 - d1024) > 3.0 / 256))), 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
