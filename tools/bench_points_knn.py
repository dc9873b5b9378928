"""KdTree k-nearest and radius queries on the MI355X: one JSON line.

  mesh:    the 549 144 vertices of the 512^3 sphere mesh (Sdfs.Sphere(1), bounds -1.5..1.5, no clip) queried with themselves,
           each moved by a fixed pseudo-random offset of up to a quarter of the vertex spacing (tools/bench_points.py's case):
           sdfk_points_search, then sdfk_points_knn for k = 1, 8, 16, 32, 64
  uniform: 10^6 uniform queries on 10^7 uniform points in [0, 1)^3: sdfk_points_search and sdfk_points_knn at k = 16
  radius:  a radius of two voxel edges on the mesh vertices: sdfk_points_radius_count and sdfk_points_radius_fill timed
           separately, with the mean and the maximum number of neighbours per query
  cpu:     scipy.spatial.cKDTree.query(k=..., workers=16) on the host for the mesh legs, left out without scipy

Every leg: the median of --reps host wall-clock times around a call that ends in a device synchronise, with min..max; device
buffers are torch tensors, so host copies are excluded.  ratio_to_search: the leg's median over the median of sdfk_points_search
on the same set and queries, measured in the same run.  candidates_per_query: static points whose distance was computed, per
query (sdfk_points_stats under sdfk_profile_enable(1), a separate call).  Kernel times come from a rocprofv3 --kernel-trace --stats
run of this script.
  python tools/bench_points_knn.py [--reps 5] [--skip-cpu] [--skip-uniform]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-uniform", action="store_true")
    ap.add_argument("--n", type=int, default=512, help="grid of the mesh")
    a = ap.parse_args()

    import torch
    import sdfkit_amd as K
    from sdfkit_amd import _native as N

    N.init(0)
    L = N.lib()
    N.bind_torch_stream()
    dev = torch.device("cuda:0")

    def sync():
        N.check(L.sdfk_synchronize())
        torch.cuda.synchronize()

    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def timed(fn):
        fn()   # warm-up
        ts = []
        for _ in range(a.reps):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(1e3 * (time.perf_counter() - t0))
        return {"ms": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}

    def candidates(h, fn):
        N.check(L.sdfk_profile_enable(1))
        fn()
        sync()
        N.check(L.sdfk_profile_enable(0))
        st = (C.c_int64 * 5)()
        N.check(L.sdfk_points_stats(h, st))
        return round(st[3] / max(1, st[4]), 2)

    def make_set(P):
        Pd = torch.from_numpy(P).to(dev)
        h = C.c_void_p()
        N.check(L.sdfk_points_create_device(p(Pd), len(P), C.byref(h)))
        return h

    def search_leg(h, Qd, n):
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        dist = torch.empty(n, dtype=torch.float32, device=dev)

        def fn():
            N.check(L.sdfk_points_search_device(h, p(Qd), n, p(idx), p(dist), None))
        res = timed(fn)
        res["candidates_per_query"] = candidates(h, fn)
        return res

    def knn_leg(h, Qd, n, k, base_ms):
        idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        dist = torch.empty((n, k), dtype=torch.float32, device=dev)
        found = torch.empty(n, dtype=torch.int32, device=dev)

        def fn():
            N.check(L.sdfk_points_knn_device(h, p(Qd), n, k, float("inf"), p(idx), p(dist), p(found)))
        res = timed(fn)
        res["candidates_per_query"] = candidates(h, fn)
        res["ratio_to_search"] = round(res["ms"] / base_ms, 3)
        return res

    out = {"metric": "points_knn", "reps": a.reps}

    # 1. the 512^3 sphere mesh's vertices, queried with themselves
    n = a.n
    mesh = K.Sdfs.Sphere(1.0).ToMesh([-1.5] * 3, [1.5] * 3, n, n, n, clipToBounds=False)
    V = np.ascontiguousarray(np.asarray(mesh.Vertices, f32).reshape(-1, 3))
    spacing = 3.0 / (n - 1)
    rs = np.random.default_rng(0)
    Qm = (V + rs.uniform(-0.25 * spacing, 0.25 * spacing, V.shape)).astype(f32)
    h = make_set(V)
    Qd = torch.from_numpy(Qm).to(dev)
    st = (C.c_int64 * 5)()
    N.check(L.sdfk_points_stats(h, st))
    leg = {"static": len(V), "queries": len(Qm), "grid": [st[0], st[1], st[2]], "search": search_leg(h, Qd, len(Qm))}
    base = leg["search"]["ms"]
    for k in (1, 8, 16, 32, 64):
        leg[f"knn_{k}"] = knn_leg(h, Qd, len(Qm), k, base)
    out["mesh"] = leg

    # 2. a radius of two voxel edges on the same vertices
    r = 2.0 * spacing
    nq = len(Qm)
    off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)

    def count():
        N.check(L.sdfk_points_radius_count_device(h, p(Qd), nq, r, p(off)))
    rc = timed(count)
    rc["candidates_per_query"] = candidates(h, count)
    rc["ratio_to_search"] = round(rc["ms"] / base, 3)
    sync()
    offs = off.cpu().numpy()
    total = int(offs[-1])
    ridx = torch.empty(total, dtype=torch.int32, device=dev)
    rdist = torch.empty(total, dtype=torch.float32, device=dev)

    def fill():
        N.check(L.sdfk_points_radius_fill_device(h, p(Qd), nq, r, p(off), p(ridx), p(rdist)))
    rf = timed(fill)
    rf["candidates_per_query"] = candidates(h, fill)
    rf["ratio_to_search"] = round(rf["ms"] / base, 3)
    out["radius"] = {"radius": round(r, 6), "radius_in_voxel_edges": 2, "queries": nq, "total_neighbours": total,
                     "neighbours_mean": round(total / nq, 2), "neighbours_max": int(np.diff(offs).max()), "count": rc, "fill": rf}
    if not a.skip_cpu:
        try:
            from scipy.spatial import cKDTree
            tree = cKDTree(V)
            cpu = {}
            for k in (1, 16, 64):
                t0 = time.perf_counter()
                tree.query(Qm, k=k, workers=16)
                cpu[f"query_k{k}_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
            t0 = time.perf_counter()
            tree.query_ball_point(Qm, r, workers=16, return_sorted=False)
            cpu["query_ball_point_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
            out["mesh"]["cpu_ckdtree_16w"] = cpu
        except ImportError:
            pass
    L.sdfk_points_free(h)
    del Qd, ridx, rdist, off

    # 3. 10^6 uniform queries on 10^7 uniform points
    if not a.skip_uniform:
        P = rs.random((10_000_000, 3), dtype=f32)
        Q = rs.random((1_000_000, 3), dtype=f32)
        h = make_set(P)
        Qd = torch.from_numpy(Q).to(dev)
        N.check(L.sdfk_points_stats(h, st))
        leg = {"static": len(P), "queries": len(Q), "grid": [st[0], st[1], st[2]], "search": search_leg(h, Qd, len(Q))}
        leg["knn_16"] = knn_leg(h, Qd, len(Q), 16, leg["search"]["ms"])
        out["uniform"] = leg
        L.sdfk_points_free(h)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
