"""Point-cloud normals and volumes on the MI355X: one JSON line (kept as profiles/pointcloud_bench.json).

  cloud:    the 549 144 vertices of the 512^3 sphere mesh (Sdfs.Sphere(1), bounds -1.5..1.5, no clip), their mesh normals
  normals:  sdfk_points_normals_device at k = 8 and 16, and sdfk_points_knn_device at the same k on the same queries (the points
            themselves) in the same run: ratio_to_knn
  volume:   sdfk_points_to_volume_device into 256^3 with a band of 4 voxels at k = 8 and 16, and sdfk_points_knn_device (found
            only) on the 256^3 cell centres with the same k and band: ratio_to_knn; known / unknown voxels
  pipeline: scan -> mesh end to end from the host arrays: KdTree, EstimateNormals (viewpoint at the centre, negated: outwards),
            ToVoxels (k = 8, band 4 voxels), Redistance, ToMesh -- the time of each step and the whole

Every leg: the median of --reps host wall-clock times around a call that ends in a device synchronise, with min..max.
  python tools/bench_pointcloud.py [--reps 5] [--n 512] [--grid 256]
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
    ap.add_argument("--n", type=int, default=512, help="grid of the mesh the cloud comes from")
    ap.add_argument("--grid", type=int, default=256, help="grid of the volume")
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

    mesh = K.Sdfs.Sphere(1.0).ToMesh([-1.5] * 3, [1.5] * 3, a.n, a.n, a.n, clipToBounds=False)
    V = np.ascontiguousarray(np.asarray(mesh.Vertices, f32).reshape(-1, 3))
    Nm = np.ascontiguousarray(np.asarray(mesh.Normals, f32).reshape(-1, 3))
    n = len(V)
    g = a.grid
    band = 4 * 3.0 / g
    out = {"metric": "pointcloud", "reps": a.reps, "points": n, "grid": g, "band_voxels": 4}

    tree = K.KdTree(V)
    h = tree.handle
    Vd = torch.from_numpy(V).to(dev)
    Nd = torch.from_numpy(Nm).to(dev)
    found = torch.empty(n, dtype=torch.int32, device=dev)
    nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
    var = torch.empty(n, dtype=torch.float32, device=dev)
    for k in (8, 16):
        knn = timed(lambda: N.check(L.sdfk_points_knn_device(h, p(Vd), n, k, float("inf"), None, None, p(found))))
        est = timed(lambda: N.check(L.sdfk_points_normals_device(h, k, float("inf"), None, 0, p(nrm), p(var))))
        est["knn_ms"] = knn["ms"]
        est["ratio_to_knn"] = round(est["ms"] / knn["ms"], 3)
        out[f"normals_{k}"] = est

    vox = K.Voxels([-1.5] * 3, [1.5] * 3, g, g, g)
    hv = vox._ensure_device(False)
    ax = (f32(-1.5) + f32(0.5) * f32(3.0 / g)) + np.arange(g, dtype=f32) * f32(3.0 / g)
    Q = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    Qd = torch.from_numpy(Q).to(dev)
    foundq = torch.empty(len(Q), dtype=torch.int32, device=dev)
    st = (C.c_int64 * 4)()
    for k in (8, 16):
        knn = timed(lambda: N.check(L.sdfk_points_knn_device(h, p(Qd), len(Q), k, band, None, None, p(foundq))))
        vol = timed(lambda: N.check(L.sdfk_points_to_volume_device(h, p(Nd), hv, k, band, None)))
        N.check(L.sdfk_points_to_volume_device(h, p(Nd), hv, k, band, st))
        vol.update(knn_ms=knn["ms"], ratio_to_knn=round(vol["ms"] / knn["ms"], 3), known=int(st[0]), unknown=int(st[1]))
        out[f"volume_{k}"] = vol
    del Qd, foundq

    # scan -> mesh, from host arrays
    steps = {}

    def pipeline():
        t = [time.perf_counter()]
        tr = K.KdTree(V)
        sync(); t.append(time.perf_counter())
        en, _ = tr.EstimateNormals(8, viewpoint=[0, 0, 0])
        t.append(time.perf_counter())
        vx = tr.ToVoxels(-en, [-1.5] * 3, [1.5] * 3, g, g, g, k=8, maxDistance=band)
        sync(); t.append(time.perf_counter())
        full = vx.Redistance()
        sync(); t.append(time.perf_counter())
        m = full.ToMesh()
        nv = len(m.Vertices)
        t.append(time.perf_counter())
        for name, d in zip(("build", "normals", "to_voxels", "redistance", "to_mesh"), np.diff(t)):
            steps.setdefault(name, []).append(1e3 * d)
        steps["vertices"] = nv
    total = timed(pipeline)
    total["steps_ms"] = {k: round(float(np.median(v)), 4) for k, v in steps.items() if k != "vertices"}
    total["vertices"] = steps["vertices"]
    out["pipeline"] = total
    N.check(L.sdfk_set_stream(None))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
