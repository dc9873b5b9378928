"""Triangle-mesh distance volumes (MeshSdf, csrc/lib_trimesh.hip) on the MI355X: one JSON line.

  sphere: the clipped 512^3 mesh of Sdfs.Sphere(1) over -1.25..1.25 -> build, and sdfk_trimesh_to_volume into 256^3 over the
          same box with the band at +inf and at 4 voxels
  box:    the 12-triangle box [-0.6, 0.6]^3 into 512^3 over -1..1
  closest: 10^6 uniform queries in the sphere box against the sphere mesh
Times are host wall clock around work that ends in a device synchronise (median of --reps, min and max given as the spread).
candidates_per_query: binary64 closest-point evaluations per query (sdfk_trimesh_stats under sdfk_profile_enable(1), a
separate run).  Kernel times come from a rocprofv3 --kernel-trace --stats run of this script.
  python tools/bench_meshsdf.py [--reps 5] [--banded-only]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--banded-only", action="store_true", help="skip the unbanded volume and the 10^6 queries (kernel traces)")
    args = ap.parse_args()
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from sdfkit_amd.meshsdf import MeshSdf
    N.init()
    L = N.lib()
    sync = lambda: L.sdfk_synchronize()  # noqa: E731
    out = {}
    m = K.Sdfs.Sphere(1.0).ToMesh([-1.25] * 3, [1.25] * 3, 512, 512, 512, clipToBounds=True)
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, np.int32)
    out["sphere_triangles"] = len(T) // 3
    out["sphere_build"] = _times(lambda: MeshSdf((V, T)), args.reps, sync)
    t = MeshSdf((V, T))
    n = args.n
    vox = K.Voxels([-1.25] * 3, [1.25] * 3, n, n, n)
    vh = vox._ensure_device(False)
    cell = 2.5 / n
    bands = (("4vox", 4 * cell),) if args.banded_only else (("inf", float("inf")), ("4vox", 4 * cell))
    for name, band in bands:
        out[f"sphere_to_volume_{n}_band_{name}"] = _times(lambda: N.check(L.sdfk_trimesh_to_volume(t.handle, vh, C.c_float(band))), args.reps, sync)
        L.sdfk_profile_enable(1)
        N.check(L.sdfk_trimesh_to_volume(t.handle, vh, C.c_float(band)))
        L.sdfk_profile_enable(0)
        st = t.stats()
        out[f"sphere_candidates_per_voxel_band_{name}"] = round(st["candidates"] / max(st["queries"], 1), 2)
        out["sphere_crossings"] = st["crossings"]
    out["sphere_grid"] = t.stats()["grid"]
    Vb, Tb = np.array([[x, y, z] for z in (-0.6, 0.6) for y in (-0.6, 0.6) for x in (-0.6, 0.6)], f32), \
        np.array([0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5], np.int32)
    tb = MeshSdf((Vb, Tb))
    vb = K.Voxels([-1] * 3, [1] * 3, 512, 512, 512)
    vbh = vb._ensure_device(False)
    out["box_to_volume_512"] = _times(lambda: N.check(L.sdfk_trimesh_to_volume(tb.handle, vbh, C.c_float(np.inf))), args.reps, sync)
    if args.banded_only:
        print(json.dumps(out))
        return
    rng = np.random.default_rng(0)
    Q = rng.uniform(-1.25, 1.25, (1_000_000, 3)).astype(f32)
    import torch
    qd = torch.from_numpy(Q).cuda()
    ti = torch.empty(len(Q), dtype=torch.int32, device="cuda")
    di = torch.empty(len(Q), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out["closest_1e6"] = _times(lambda: N.check(L.sdfk_trimesh_closest_device(t.handle, C.c_void_p(qd.data_ptr()), len(Q), C.c_void_p(ti.data_ptr()),
                                                                               C.c_void_p(di.data_ptr()), None)), args.reps,
                                lambda: (sync(), torch.cuda.synchronize()))
    L.sdfk_profile_enable(1)
    N.check(L.sdfk_trimesh_closest_device(t.handle, C.c_void_p(qd.data_ptr()), len(Q), C.c_void_p(ti.data_ptr()), C.c_void_p(di.data_ptr()), None))
    L.sdfk_profile_enable(0)
    st = t.stats()
    out["closest_candidates_per_query"] = round(st["candidates"] / max(st["queries"], 1), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
