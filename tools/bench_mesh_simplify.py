"""Mesh simplification (MeshSdf.Simplify, csrc/lib_trimesh_simplify.hip) on the MI355X: one JSON line, also written to
profiles/mesh_simplify_bench.json.

  The clipped 512^3 marching-cubes mesh of Sdfs.Sphere(1) over -1.25..1.25 (790 728 vertices, 1.58 M triangles) under a cellSize
  of 2, 4 and 8 voxels and each placement (representative, centroid, quadric), duplicates "one":
    sdfk_trimesh_simplify_device into device buffers on a handle made before the clock starts (and, for the quadric, after one
    call that made the handle's corner lists: the warm-up); the counts, the stats and, from one further call under the library's
    event profile (sdfk_profile_enable(1)), the time inside each bracketed scope -- k_ts_place is the placement kernel, k_rs_pass
    one radix pass (histogram, scan, scatter), k_tw_* the grouping shared with welding.
  The yardstick, per cell size: sdfk_trimesh_weld_device at the same tolerance on the same mesh -- the same grouping, no triangle
  sort and no placement.
These are WHOLE-CALL times: host wall clock around a call that ends in a device synchronise (the calls synchronise themselves),
median of --reps after one warm-up, min and max as the spread.
  python tools/bench_mesh_simplify.py [--reps 5] [--n 512]
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
PLACEMENTS = ("representative", "centroid", "quadric")


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


def _profiled(call, sync, N):
    L = N.lib()
    N.check(L.sdfk_profile_reset()); N.check(L.sdfk_profile_enable(1))
    call()
    sync()
    N.check(L.sdfk_profile_enable(0))
    return {k: round(v[0], 3) for k, v in N.profile_snapshot().items() if v[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=512, help="the grid of the sphere mesh")
    args = ap.parse_args()
    import torch
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from sdfkit_amd.meshsdf import MeshSdf
    N.init()
    L = N.lib()
    sync = lambda: (L.sdfk_synchronize(), torch.cuda.synchronize())  # noqa: E731
    m = K.Sdfs.Sphere(1.0).ToMesh([-1.25] * 3, [1.25] * 3, args.n, args.n, args.n, clipToBounds=True)
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, np.int32)
    nv, nt = len(V), len(T) // 3
    dev = torch.device("cuda", N._inited_device or 0)
    ints = [torch.empty(k, dtype=torch.int32, device=dev) for k in (nv, nv, nt, 3 * nt)]
    floats = [torch.empty((nv, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    ptrs = [C.c_void_p(b.data_ptr()) for b in ints + floats]
    t = MeshSdf((V, T))
    sync()
    voxel = 2.5 / args.n
    out = {"vertices": nv, "triangles": nt, "voxel": voxel, "cells": {}}
    for voxels in (2, 4, 8):
        cell = float(f32(voxels * voxel))
        row = {"cellSize": cell}
        kv, kt, st4 = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
        weld = lambda: N.check(L.sdfk_trimesh_weld_device(t.handle, C.c_float(cell), 0, *ptrs, C.byref(kv), C.byref(kt), st4))  # noqa: E731
        row["weld"] = _times(weld, args.reps, sync)
        row["weld"].update({"vertices_out": kv.value, "triangles_out": kt.value, "passes": int(st4[3]), "profiled_scopes_ms": _profiled(weld, sync, N)})
        for code, name in enumerate(PLACEMENTS):
            st = (C.c_int64 * 6)()
            call = lambda: N.check(L.sdfk_trimesh_simplify_device(t.handle, C.c_float(cell), code, 0, *ptrs, C.byref(kv), C.byref(kt), st))  # noqa: E731
            r = _times(call, args.reps, sync)
            r.update({"vertices_out": kv.value, "triangles_out": kt.value, "merged": int(st[0]), "degenerate_dropped": int(st[1]),
                      "duplicates_dropped": int(st[2]), "unreferenced_dropped": int(st[3]), "passes": int(st[4]), "quadric_fallbacks": int(st[5]),
                      "profiled_scopes_ms": _profiled(call, sync, N)})
            r["times_weld"] = round(r["median_ms"] / row["weld"]["median_ms"], 2)
            row[name] = r
        out["cells"][str(voxels)] = row
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_simplify_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
