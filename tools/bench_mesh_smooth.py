"""Mesh adjacency, smoothing and vertex normals (MeshSdf.Adjacency / Smooth / VertexNormals, csrc/lib_trimesh_smooth.hip) on the
MI355X: one JSON line, also written to profiles/mesh_smooth_bench.json.

  sphere: the clipped 512^3 mesh of Sdfs.Sphere(1) over -1.25..1.25 (790 728 vertices, 1.58 M triangles)
  many:   a RepeatXY lattice of small spheres at 256 x 256 x 32 (121 closed components)
  per mesh:
    adjacency_first   the first sdfk_trimesh_adjacency_device of a fresh handle (records, sort, heads, scans; it synchronises
                      twice to size the arrays), a fresh handle per repetition
    smooth_10         sdfk_trimesh_smooth_device, 10 Taubin iterations (20 steps) on a handle that has its adjacency
    normals_first     the first sdfk_trimesh_vertex_normals_device of a fresh handle (the corner sort included)
    normals           the same call on a handle that has its corners
    Next to each of smooth_10 and normals: the bytes the call must move and that over its median time as a fraction of the 8 TB/s
    peak.  A step reads nbr_start (4 (nv + 1)), nbr (4 E), a boundary byte per vertex, gathers 12 bytes per neighbour (12 E; they
    come from cache: the positions are 12 nv bytes) and its own position, and stores 12 nv.  `bytes_gathered` counts every gather,
    `bytes_compulsory` counts the position array once per step.
    scipy_host        where scipy is importable: the same ten iterations as sparse matrix products in binary64 on the host (the
                      matrix build apart), for context; its sums run in another order, so its bits differ
Times are host wall clock around work that ends in a device synchronise (median of --reps after one warm-up call of the same
shape, min and max given as the spread).
  python tools/bench_mesh_smooth.py [--reps 5] [--n 512]
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
PEAK = 8e12
ITERATIONS, LAMBDA, MU = 10, 0.5, -0.53


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


def _with_bytes(times, gathered, compulsory):
    s = times["median_ms"] * 1e-3
    times.update({"bytes_gathered": int(gathered), "bytes_compulsory": int(compulsory),
                  "peak_fraction_gathered": round(gathered / s / PEAK, 4), "peak_fraction_compulsory": round(compulsory / s / PEAK, 4)})
    return times


def _scipy_ms(V, adj):
    try:
        from scipy.sparse import csr_matrix
    except Exception:
        return None
    nv = len(V)
    t0 = time.perf_counter()
    deg = np.maximum(adj.Degree, 1).astype(np.float64)
    A = csr_matrix((np.repeat(1.0 / deg, adj.Degree), adj.Neighbors.astype(np.int64), adj.Start.astype(np.int64)), shape=(nv, nv))
    free = ((adj.Degree > 0) & (adj.Boundary == 0)).astype(np.float64)[:, None]
    build = (time.perf_counter() - t0) * 1e3
    P = V.astype(np.float64)
    t0 = time.perf_counter()
    for _ in range(ITERATIONS):
        for s in (LAMBDA, MU):
            P = (P + free * (s * (A @ P - P))).astype(f32).astype(np.float64)
    return {"ms": round((time.perf_counter() - t0) * 1e3, 3), "matrix_build_ms": round(build, 3)}


def _bench(V, T, cols, reps, sync, torch, N):
    from sdfkit_amd.meshsdf import SMOOTH_PIN_BOUNDARY, MeshSdf
    L = N.lib()
    dev = torch.device("cuda", N._inited_device or 0)
    nv, nt = len(V), len(T) // 3
    out = {"vertices": nv, "triangles": nt}
    pos, nrm = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nv, 3), dtype=torch.float32, device=dev)
    start, bnd = torch.empty(nv + 1, dtype=torch.int32, device=dev), torch.empty(nv, dtype=torch.uint8, device=dev)
    nbr = torch.empty(6 * nt, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    handles = [MeshSdf((V, T, cols)) for _ in range(reps + 1)]
    fresh, fresh_normals = iter(handles), iter(handles)
    n = C.c_int64()
    adj = lambda h: N.check(L.sdfk_trimesh_adjacency_device(h.handle, C.c_void_p(start.data_ptr()), C.c_void_p(nbr.data_ptr()),  # noqa: E731
                                                            C.c_void_p(bnd.data_ptr()), C.byref(n)))
    out["adjacency_first"] = _times(lambda: adj(next(fresh)), reps, sync)
    E = n.value
    t = handles[0]
    a = t.Adjacency()
    out["entries"], out["max_degree"], out["boundary_vertices"] = E, int(a.Degree.max()), int(np.count_nonzero(a.Boundary))
    steps = 2 * ITERATIONS
    smooth = lambda: N.check(L.sdfk_trimesh_smooth_device(t.handle, ITERATIONS, C.c_float(LAMBDA), C.c_float(MU), SMOOTH_PIN_BOUNDARY,  # noqa: E731
                                                          C.c_void_p(pos.data_ptr())))
    fixed = 4 * (nv + 1) + 4 * E + nv + 12 * nv      # nbr_start, nbr, the boundary bytes, the store
    out["smooth_10"] = _with_bytes(_times(smooth, reps, sync), steps * (fixed + 12 * E + 12 * nv), steps * (fixed + 12 * nv))
    normals = lambda h: N.check(L.sdfk_trimesh_vertex_normals_device(h.handle, C.c_void_p(pos.data_ptr()), 0, C.c_void_p(nrm.data_ptr())))  # noqa: E731
    out["normals_first"] = _times(lambda: normals(next(fresh_normals)), reps, sync)
    corners = 3 * nt
    fixed = 4 * (nv + 1) + 4 * corners + 12 * nv    # inc_start, inc, the store
    out["normals"] = _with_bytes(_times(lambda: normals(t), reps, sync), fixed + corners * (12 + 36), fixed + 12 * nt + 12 * nv)
    out["scipy_host"] = _scipy_ms(V, a)
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
    out["sphere"] = _bench(V, T, (0.5 + 0.4 * V).astype(f32), args.reps, sync, torch, N)
    lattice = K.SdfExprs.Sphere(0.06).RepeatXY(0.2, 0.2).ToSdf().ToMesh([-1.0, -1.0, -0.1], [1.0, 1.0, 0.1], args.n // 2, args.n // 2, max(args.n // 16, 8))
    V, T = np.array(lattice.Vertices, f32), np.array(lattice.Triangles, np.int32)
    out["many"] = _bench(V, T, None, args.reps, sync, torch, N)
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_smooth_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
