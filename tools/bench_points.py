"""KdTree / IterativeClosestPoint on the MI355X: one JSON line.

  mesh:    build + search of the 549 144 vertices of the 512^3 sphere mesh (Sdfs.Sphere(1), bounds -1.5..1.5, no clip)
           queried with themselves, each moved by a fixed pseudo-random offset of up to a quarter of the vertex spacing
  uniform: build on 10^7 uniform points in [0, 1)^3, search of 10^6 uniform queries
  icp:     registration of the union8 mesh at 512^3 onto itself after RotationX(2 deg) * Translation(0, 0.05, 0), on device
  cpu:     the same searches with scipy.spatial.cKDTree (16 workers) on the host, null without scipy

Times are host wall clock around work that ends in a device synchronise (median of --reps); device buffers are torch tensors,
so the search times exclude host copies.  candidates_per_query: static points whose distance was computed, per query
(sdfk_points_stats under sdfk_profile_enable(1), a separate run).  Kernel times come from a rocprofv3 --kernel-trace --stats
run of this script.
  python tools/bench_points.py [--reps 5] [--skip-cpu]
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


def _median_ms(fn, reps, sync):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--n", type=int, default=512, help="grid of the meshes")
    a = ap.parse_args()

    import torch
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from sdfkit_amd.raymarch import Matrix4x4
    from tests import scenes as S

    N.init(0)
    L = N.lib()
    N.bind_torch_stream()
    dev = torch.device("cuda:0")

    def sync():
        N.check(L.sdfk_synchronize())
        torch.cuda.synchronize()

    out = {"metric": "points", "reps": a.reps}

    def search_case(name, P, Q):
        Pd = torch.from_numpy(P).to(dev)
        Qd = torch.from_numpy(Q).to(dev)
        idx = torch.empty(len(Q), dtype=torch.int32, device=dev)
        dist = torch.empty(len(Q), dtype=torch.float32, device=dev)
        holder = {}

        def build():
            h = C.c_void_p()
            N.check(L.sdfk_points_create_device(C.c_void_p(Pd.data_ptr()), len(P), C.byref(h)))
            if "h" in holder:
                L.sdfk_points_free(holder["h"])
            holder["h"] = h

        def search():
            N.check(L.sdfk_points_search_device(holder["h"], C.c_void_p(Qd.data_ptr()), len(Q), C.c_void_p(idx.data_ptr()),
                                                C.c_void_p(dist.data_ptr()), None))
        build()
        search()   # warm-up
        b_ms, _ = _median_ms(build, a.reps, sync)
        s_ms, s_all = _median_ms(search, a.reps, sync)
        N.check(L.sdfk_profile_enable(1))
        search()
        sync()
        N.check(L.sdfk_profile_enable(0))
        st = (C.c_int64 * 5)()
        N.check(L.sdfk_points_stats(holder["h"], st))
        L.sdfk_points_free(holder["h"])
        res = {"static": len(P), "queries": len(Q), "build_ms": round(b_ms, 4), "search_ms": round(s_ms, 4),
               "search_ms_all": [round(t, 4) for t in s_all], "build_plus_search_ms": round(b_ms + s_ms, 4),
               "grid": [st[0], st[1], st[2]], "candidates_per_query": round(st[3] / max(1, st[4]), 2)}
        if not a.skip_cpu:
            try:
                from scipy.spatial import cKDTree
                t0 = time.perf_counter()
                tree = cKDTree(P)
                t1 = time.perf_counter()
                tree.query(Q, k=1, workers=16)
                t2 = time.perf_counter()
                res["cpu_ckdtree_16w"] = {"build_ms": round(1e3 * (t1 - t0), 2), "search_ms": round(1e3 * (t2 - t1), 2)}
            except ImportError:
                res["cpu_ckdtree_16w"] = None
        out[name] = res

    # 1. the 512^3 sphere mesh's vertices
    n = a.n
    mesh = K.Sdfs.Sphere(1.0).ToMesh([-1.5] * 3, [1.5] * 3, n, n, n, clipToBounds=False)
    V = np.ascontiguousarray(np.asarray(mesh.Vertices, f32).reshape(-1, 3))
    spacing = 3.0 / (n - 1)
    rs = np.random.default_rng(0)
    Qm = (V + rs.uniform(-0.25 * spacing, 0.25 * spacing, V.shape)).astype(f32)
    search_case("mesh", V, Qm)
    # 2. 10^6 uniform queries against 10^7 uniform points
    search_case("uniform", rs.random((10_000_000, 3), dtype=f32), rs.random((1_000_000, 3), dtype=f32))

    # 3. ICP: union8 at 512^3
    _, sdf = S.CATALOGUE["union8"]()
    m8 = sdf.ToMesh([-2.5] * 3, [2.5] * 3, n, n, n, clipToBounds=False)
    V8 = np.ascontiguousarray(np.asarray(m8.Vertices, f32).reshape(-1, 3))
    xf = Matrix4x4.Multiply(Matrix4x4.CreateRotationX(np.float32(2.0) * np.float32(np.pi) / np.float32(180.0)),
                            Matrix4x4.CreateTranslation(0, np.float32(0.05), 0))
    from tests.points_model import transform_points
    moved = transform_points(V8, xf)
    icp = K.IterativeClosestPoint(V8)
    D = torch.from_numpy(moved).to(dev)
    icp.RegisterDevicePoints(D.data_ptr(), len(moved))   # warm-up
    calls = []
    for _ in range(a.reps):
        D.copy_(torch.from_numpy(moved))
        sync()
        t0 = time.perf_counter()
        icp.RegisterDevicePoints(D.data_ptr(), len(moved))
        sync()
        calls.append(1e3 * (time.perf_counter() - t0))
    c_ms = float(np.median(calls))
    out["icp"] = {"points": len(moved), "iterations": icp.Iterations, "call_ms": round(c_ms, 4),
                  "ms_per_iteration": round(c_ms / max(1, icp.Iterations), 4), "call_ms_all": [round(t, 4) for t in calls]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
