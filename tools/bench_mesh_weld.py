"""Mesh welding (MeshSdf.Weld, csrc/lib_trimesh_weld.hip) on the MI355X: one JSON line, also written to
profiles/mesh_weld_bench.json.

  The clipped 512^3 mesh of Sdfs.Sphere(1) over -1.25..1.25 (790 728 vertices, 1.58 M triangles), three ways and a fourth for the pass skipping:
    identity      as it is: indexed, no two equal positions -- nothing merges, the mesh comes back
    soup          de-indexed to three vertices per triangle (4.7 M vertices), exact mode: welds back to the indexed count
    soup_lattice  the same soup, lattice mode with a cell far below the mesh's spacing
    soup_offset   the same soup moved by (5.5, 5.5, 5.5), exact mode: every coordinate lies in 4.25 .. 6.75, one binade, so the keys
                  share their top byte and the pass skipping has something to skip (the sphere round the origin has both signs
                  and every exponent: all 12 bytes differ)
  per case: sdfk_trimesh_weld_device into device buffers on a handle made before the clock starts; the counts, what merged, the
  radix passes run (of up to 12 in exact mode, 8 in lattice mode) and, from one further call under the library's event profile
  (sdfk_profile_enable(1)), the time inside each bracketed scope: k_rs_pass is one radix pass (histogram, scan, scatter), so
  `skipped_passes_ms_estimate` = (most passes - passes run) x the mean k_rs_pass -- an estimate, not a measured second build.
  numpy_unique_host: np.unique(axis=0, return_index, return_inverse) of the soup's positions on the host, for context.
These are WHOLE-CALL times: host wall clock around a call that ends in a device synchronise (the call synchronises itself: pass
masks and counts come back to the host), median of --reps after one warm-up, min and max as the spread.  No per-kernel trace.
  python tools/bench_mesh_weld.py [--reps 5] [--n 512]
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


def _bench(V, T, tolerance, most_passes, reps, sync, torch, N):
    from sdfkit_amd.meshsdf import MeshSdf
    L = N.lib()
    dev = torch.device("cuda", N._inited_device or 0)
    nv, nt = len(V), len(T) // 3
    ints = [torch.empty(k, dtype=torch.int32, device=dev) for k in (nv, nv, nt, 3 * nt)]
    floats = [torch.empty((nv, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    t = MeshSdf((V, T))
    sync()
    kv, kt, st = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
    call = lambda: N.check(L.sdfk_trimesh_weld_device(t.handle, C.c_float(tolerance), 0, *[C.c_void_p(b.data_ptr()) for b in ints + floats],  # noqa: E731
                                                      C.byref(kv), C.byref(kt), st))
    out = {"vertices": nv, "triangles": nt, "tolerance": tolerance}
    out.update(_times(call, reps, sync))
    out.update({"vertices_out": kv.value, "triangles_out": kt.value, "merged": int(st[0]), "degenerate_dropped": int(st[1]),
                "unreferenced_dropped": int(st[2]), "passes": int(st[3]), "most_passes": most_passes})
    N.check(L.sdfk_profile_reset()); N.check(L.sdfk_profile_enable(1))
    call()
    sync()
    N.check(L.sdfk_profile_enable(0))
    prof = {k: (v[0], v[1]) for k, v in N.profile_snapshot().items() if v[1]}
    out["profiled_scopes_ms"] = {k: round(v[0], 3) for k, v in prof.items()}
    if "k_rs_pass" in prof:
        per = prof["k_rs_pass"][0] / prof["k_rs_pass"][1]
        out["radix_pass_mean_ms"] = round(per, 3)
        out["skipped_passes_ms_estimate"] = round((most_passes - int(st[3])) * per, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=512, help="the grid of the sphere mesh")
    args = ap.parse_args()
    import torch
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    N.init()
    L = N.lib()
    sync = lambda: (L.sdfk_synchronize(), torch.cuda.synchronize())  # noqa: E731
    m = K.Sdfs.Sphere(1.0).ToMesh([-1.25] * 3, [1.25] * 3, args.n, args.n, args.n, clipToBounds=True)
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, np.int32)
    S, ST = np.ascontiguousarray(V[T]), np.arange(len(T), dtype=np.int32)
    out = {"identity": _bench(V, T, 0.0, 12, args.reps, sync, torch, N), "soup": _bench(S, ST, 0.0, 12, args.reps, sync, torch, N),
           "soup_lattice": _bench(S, ST, 2.5 / args.n / 256, 8, args.reps, sync, torch, N),
           "soup_offset": _bench(S + f32(5.5), ST, 0.0, 12, args.reps, sync, torch, N)}
    t0 = time.perf_counter()
    _, first, inverse = np.unique(S, axis=0, return_index=True, return_inverse=True)
    out["numpy_unique_host"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "groups": int(len(first))}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_weld_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
