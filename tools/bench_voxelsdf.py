"""Voxel volumes inside SDF programs (Voxels.ToSdf, sdfk_program_create_bound) on the MI355X: one JSON line.

  build:   the clipped 512^3 mesh of a coloured sphere (SdfExprs.Sphere(1, colour)) over -1.25..1.25 -> MeshSdf -> a banded
           (4 voxels) 256^3 volume with colours over the same box -> vox.ToSdf() (trilinear, colours) -> program creation
           (snapshot copy + min/max pyramids of the four channels)
  sample:  that SDF sampled into a 512^3 colour volume (Voxels.SampleSdf, 16 B per voxel stored), and for comparison the one-
           primitive colour sampler (SdfExprs.Sphere(1, colour)) into the same volume; fraction of the 8 TB/s peak on the stored bytes
  mesh:    min(vox.ToSdf(), Sdfs.Box) -> ToMesh at 512^3, stored volume (SDFK_OPT_ELIDE_VOLUME = 0) and product default (2)
  image:   one 1920 x 1080 RayMarcher frame (depth + colour) of the same union
  points:  10^6 uniform points through SdfEx.Sample
Times are host wall clock around work that ends in a device synchronise (median of --reps, min and max as the spread).
Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script.
  python tools/bench_voxelsdf.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

f32 = np.float32
PEAK_TBS = 8.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from sdfkit_amd.api import Sdf, _box_distance
    from sdfkit_amd.expr import MathF, Vec3, Vec4
    N.init()
    L = N.lib()
    sync = lambda: L.sdfk_synchronize()  # noqa: E731
    out = {}
    box = [-1.25] * 3, [1.25] * 3
    colored = K.SdfExprs.Sphere(1.0, (0.25, 0.5, 0.75)).ToSdf()
    m = colored.ToMesh(*box, 512, 512, 512, clipToBounds=True)
    V, T, Cc = np.array(m.Vertices, f32), np.array(m.Triangles, np.int32), np.array(m.Colors, f32)
    t = K.MeshSdf((V, T, Cc))
    vox = K.Voxels(*box, 256, 256, 256)
    t.SampleInto(vox, 4 * 2.5 / 256)
    sdf = vox.ToSdf()
    out["mesh_triangles"] = len(T) // 3

    def bind():
        sdf._destroy()
        sdf.program()
    out["bind_256_4ch"] = _times(bind, args.reps, sync)

    # 1. the sampler, 512^3 with colours
    dst = K.Voxels([-1.5] * 3, [1.5] * 3, 512, 512, 512)
    dh = dst._ensure_device(True)
    stored = 512 ** 3 * 16
    prog = sdf.program()
    out["sample_512_vox"] = _times(lambda: N.check(L.sdfk_sample(prog, dh, 0)), args.reps, sync)
    sp = colored.program()
    out["sample_512_sphere_color"] = _times(lambda: N.check(L.sdfk_sample(sp, dh, 0)), args.reps, sync)
    for k in ("sample_512_vox", "sample_512_sphere_color"):
        out[k]["peak_fraction"] = round(stored / (out[k]["median_ms"] * 1e-3) / (PEAK_TBS * 1e12), 3)
    out["sample_vox_over_sphere"] = round(out["sample_512_vox"]["median_ms"] / out["sample_512_sphere_color"]["median_ms"], 2)
    del dst

    # 2. a union with a box, meshed at 512^3
    def fn(p):
        v = vox.Sample(p)
        c = vox.SampleColor(p)
        q = Vec3(p.x - 0.9, p.y, p.z)
        return Vec4(c.x, c.y, c.z, MathF.Min(v, _box_distance(q, (0.3, 0.6, 0.4))))
    union = Sdf(fn, True)
    for mode, name in ((0, "stored"), (2, "default")):
        with N.option(N.OPT_ELIDE_VOLUME, mode):
            out[f"tomesh_512_{name}"] = _times(lambda: union.ToMesh([-1.5] * 3, [1.5] * 3, 512, 512, 512).Vertices, args.reps, sync)
    out["tomesh_512_vertices"] = len(union.ToMesh([-1.5] * 3, [1.5] * 3, 512, 512, 512).Vertices)

    # 3. one 1920 x 1080 frame
    rm = K.RayMarcher(1920, 1080, union)
    out["raymarch_1920x1080"] = _times(lambda: rm.Render(), args.reps, sync)

    # 4. 10^6 points
    rng = np.random.default_rng(0)
    Q = rng.uniform(-1.5, 1.5, (1_000_000, 3)).astype(f32)
    res = np.zeros((len(Q), 4), f32)
    out["eval_points_1e6"] = _times(lambda: union.Sample(Q, res), args.reps, sync)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
