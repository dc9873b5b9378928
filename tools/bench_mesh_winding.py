"""The generalized winding number of triangle meshes (MeshSdf.WindingNumber / ToVoxels(sign="winding"), csrc/lib_trimesh_winding.hip)
on the MI355X: one JSON line, also written to profiles/mesh_winding_bench.json.

  The clipped 512^3 marching-cubes mesh of Sdfs.Sphere(1) over -1.25..1.25 (1.58 M triangles), the mesh the other mesh tools use:
    build        the hierarchy: the first sdfk_trimesh_winding_device call of a fresh handle with one query (the handle itself is
                 made before the clock starts), one handle per repetition
    points       sdfk_trimesh_winding_device, 2 M queries uniform in the box, both outputs, at the default beta
    volume       sdfk_trimesh_to_volume_signed into 256^3 with a band of three voxels: SDFK_TRIMESH_SIGN_WINDING, and
                 SDFK_TRIMESH_SIGN_PARITY on the same handle (the existing function: the yardstick)
  Each figure is the median over --reps timed blocks, min and max as the spread; a block is --calls calls on device buffers ended by
  one device synchronise, host wall clock, after one warm-up block.  terms_per_query is (stats[4] + stats[5]) / stats[6] of one further
  call under sdfk_profile_enable(1): the cluster and triangle terms per query, which does not depend on clocks.
  python tools/bench_mesh_winding.py [--reps 7] [--calls 2] [--n 512] [--points 2000000] [--grid 256]
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


def _summary(ts, items):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"median_ms": round(med, 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "per_second": round(items / (med * 1e-3))}


def _blocks(fn, reps, calls, sync, items):
    for _ in range(calls):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3 / calls)
    return _summary(ts, items)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--n", type=int, default=512, help="the grid of the sphere mesh")
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--grid", type=int, default=256, help="the volume")
    args = ap.parse_args()
    import torch
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from sdfkit_amd.meshsdf import DEFAULT_WINDING_BETA, MeshSdf
    N.init()
    L = N.lib()
    sync = lambda: (L.sdfk_synchronize(), torch.cuda.synchronize())  # noqa: E731
    m = K.Sdfs.Sphere(1.0).ToMesh([-1.25] * 3, [1.25] * 3, args.n, args.n, args.n, clipToBounds=True)
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, np.int32)
    dev = torch.device("cuda", N._inited_device or 0)
    beta = DEFAULT_WINDING_BETA
    out = {"triangles": len(T) // 3, "beta": beta, "reps": args.reps, "calls_per_block": args.calls}

    # ---- the hierarchy
    one = torch.zeros((1, 3), dtype=torch.float32, device=dev)
    w1 = torch.empty(1, dtype=torch.float32, device=dev)
    ts = []
    for _ in range(args.reps + 1):
        fresh = MeshSdf((V, T))
        sync()
        t0 = time.perf_counter()
        fresh.WindingNumberDevice(one.data_ptr(), 1, beta, w1.data_ptr(), None)
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
        t = fresh
    out["build"] = _summary(ts[1:], len(T) // 3)   # (the first is the warm-up)
    s = t.winding_stats()
    out["hierarchy"] = {k: s[k] for k in ("levels", "nodes", "occupied_nodes", "largest_leaf")}
    print("build", out["build"], out["hierarchy"], file=sys.stderr, flush=True)

    def terms_per(call):
        N.check(L.sdfk_profile_enable(1))
        call()
        sync()
        N.check(L.sdfk_profile_enable(0))
        s = t.winding_stats()
        return {"cluster_terms_per_query": round(s["cluster_terms"] / max(s["queries"], 1), 2),
                "triangle_terms_per_query": round(s["triangle_terms"] / max(s["queries"], 1), 2),
                "terms_per_query": round((s["cluster_terms"] + s["triangle_terms"]) / max(s["queries"], 1), 2)}

    # ---- point queries
    n = args.points
    rng = np.random.default_rng(1)
    q = torch.from_numpy(rng.uniform(-1.25, 1.25, (n, 3)).astype(f32)).to(dev)
    w = torch.empty(n, dtype=torch.float32, device=dev)
    inside = torch.empty(n, dtype=torch.uint8, device=dev)
    sync()
    points = lambda: t.WindingNumberDevice(q.data_ptr(), n, beta, w.data_ptr(), inside.data_ptr())  # noqa: E731
    out["points"] = _blocks(points, args.reps, args.calls, sync, n)
    out["points"].update(terms_per(points))
    out["points"]["queries"] = n
    out["points"]["inside_fraction"] = round(float(inside.float().mean().item()), 4)
    print("points", out["points"], file=sys.stderr, flush=True)

    # ---- the banded volume, both signs on the one handle
    g = args.grid
    vox = K.Voxels([-1.25] * 3, [1.25] * 3, g, g, g)
    h = vox._ensure_device(False)
    band = C.c_float(3 * 2.5 / g)
    for name, mode in (("volume_winding", 1), ("volume_parity", 0)):
        call = lambda: N.check(L.sdfk_trimesh_to_volume_signed(t.handle, h, band, mode, C.c_float(beta)))  # noqa: E731
        out[name] = _blocks(call, args.reps, args.calls, sync, g ** 3)
        if mode:
            out[name].update(terms_per(call))
        print(name, out[name], file=sys.stderr, flush=True)
    out["volume_winding"]["grid"] = g
    out["volume_winding"]["times_parity"] = round(out["volume_winding"]["median_ms"] / out["volume_parity"]["median_ms"], 2)
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_winding_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
