"""Mesh topology (MeshSdf.Components / Topology / Select, csrc/lib_trimesh_topology.hip) on the MI355X: one JSON line, also
written to profiles/mesh_topology_bench.json.

  sphere: the clipped 512^3 mesh of Sdfs.Sphere(1) over -1.25..1.25 (1.58 M triangles, one closed component)
  many:   a RepeatXY lattice of small spheres at 256 x 256 x 32 (121 closed components)
  per mesh:
    components_first   the first sdfk_trimesh_components_device of a fresh handle (the label rounds; with hook rounds and
                       shortcut launches), a fresh handle per repetition
    components_cached  the same call on a handle that has its labels (two device-to-device copies)
    topology           sdfk_trimesh_topology_device, every call (records, sort, census, rows); the first one also makes the
                       sampling weights and is timed apart as topology_first
    select             sdfk_trimesh_select_device keeping every second component (or the one there is)
    scipy_host         where scipy is importable: scipy.sparse.csgraph.connected_components on the same mesh on the host
                       (building the sparse matrix included), for context
Times are host wall clock around work that ends in a device synchronise (median of --reps after one warm-up call of the same
shape, min and max given as the spread).
  python tools/bench_mesh_topology.py [--reps 5] [--n 512]
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


def _times(fn, reps, sync, warm=True):
    if warm:
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


def _scipy_ms(V, T):
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except Exception:
        return None
    T = T.reshape(-1, 3)
    t0 = time.perf_counter()
    g = coo_matrix((np.ones(2 * len(T), np.int8), (np.concatenate([T[:, 0], T[:, 1]]), np.concatenate([T[:, 1], T[:, 2]]))), shape=(len(V), len(V)))
    n, _ = connected_components(g, directed=False)
    return {"ms": round((time.perf_counter() - t0) * 1e3, 3), "components_with_unreferenced": int(n)}


def _bench(name, V, T, cols, reps, sync, torch, N):
    from sdfkit_amd.meshsdf import MeshSdf
    L = N.lib()
    dev = torch.device("cuda", N._inited_device or 0)
    nv, nt = len(V), len(T) // 3
    out = {"vertices": nv, "triangles": nt}
    vl, tl = torch.empty(nv, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    handles = [MeshSdf((V, T, cols)) for _ in range(reps + 1)]
    fresh = iter(handles)
    n, st, census = C.c_int64(), (C.c_int64 * 4)(), (C.c_int64 * 8)()
    comp = lambda h: N.check(L.sdfk_trimesh_components_device(h.handle, C.c_void_p(vl.data_ptr()), C.c_void_p(tl.data_ptr()), C.byref(n), st))  # noqa: E731
    out["components_first"] = _times(lambda: comp(next(fresh)), reps, sync)
    out["components"], out["hook_rounds"], out["shortcut_launches"] = n.value, int(st[0]), int(st[1])
    t = handles[0]
    out["components_cached"] = _times(lambda: comp(t), reps, sync)
    rows = torch.empty((max(n.value, 1), 8), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    topo = lambda h: N.check(L.sdfk_trimesh_topology_device(h.handle, census, C.c_void_p(rows.data_ptr()), n.value))  # noqa: E731
    firsts = iter(handles[1:])
    out["topology_first"] = _times(lambda: topo(next(firsts)), reps - 1, sync) if reps > 1 else None
    out["topology"] = _times(lambda: topo(t), reps, sync)
    out["census"] = [int(x) for x in census]
    keep = torch.from_numpy((np.arange(max(n.value, 1)) % 2 == 0).astype(np.uint8)).to(dev)
    vi, ti, tr = torch.empty(nv, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.int32, device=dev), torch.empty(3 * nt, dtype=torch.int32, device=dev)
    vs, cs = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nv, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    kv, kt = C.c_int64(), C.c_int64()
    out["select"] = _times(lambda: N.check(L.sdfk_trimesh_select_device(t.handle, C.c_void_p(keep.data_ptr()), *[C.c_void_p(b.data_ptr()) for b in (vi, ti, tr, vs, cs)],
                                                                        C.byref(kv), C.byref(kt))), reps, sync)
    out["selected"] = [kv.value, kt.value]
    out["scipy_host"] = _scipy_ms(V, T)
    del handles
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
    out = {}
    m = K.Sdfs.Sphere(1.0).ToMesh([-1.25] * 3, [1.25] * 3, args.n, args.n, args.n, clipToBounds=True)
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, np.int32)
    out["sphere"] = _bench("sphere", V, T, (0.5 + 0.4 * V).astype(f32), args.reps, sync, torch, N)
    lattice = K.SdfExprs.Sphere(0.06).RepeatXY(0.2, 0.2).ToSdf().ToMesh([-1.0, -1.0, -0.1], [1.0, 1.0, 0.1], args.n // 2, args.n // 2, max(args.n // 16, 8))
    V, T = np.array(lattice.Vertices, f32), np.array(lattice.Triangles, np.int32)
    out["many"] = _bench("many", V, T, None, args.reps, sync, torch, N)
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_topology_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
