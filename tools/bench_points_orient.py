"""The consistent orientation of normals on the MI355X: one JSON line (kept as profiles/points_orient_bench.json).

  cloud:    the 549 144 vertices of the 512^3 sphere mesh (Sdfs.Sphere(1), bounds -1.5..1.5, no clip), as tools/bench_pointcloud.py
  normals:  sdfk_points_normals_device at k = 8 without a viewpoint
  orient:   sdfk_points_orient_normals_device at k = 8 on a fresh copy of those normals each time (the copy is outside the
            timed region); the rounds and seeds of the call, the fraction of normals that point outward before and after, and
            ratio_to_normals: its time over the normals' in the same run

Every leg: the median of --reps host wall-clock times around a call that ends in a device synchronise, with min..max.
  python tools/bench_points_orient.py [--reps 5] [--n 512] [--k 8]
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
    ap.add_argument("--k", type=int, default=8)
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

    def timed(fn, before=lambda: None):
        before()
        fn()   # warm-up
        ts = []
        for _ in range(a.reps):
            before()
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(1e3 * (time.perf_counter() - t0))
        return {"ms": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}

    mesh = K.Sdfs.Sphere(1.0).ToMesh([-1.5] * 3, [1.5] * 3, a.n, a.n, a.n, clipToBounds=False)
    V = np.ascontiguousarray(np.asarray(mesh.Vertices, f32).reshape(-1, 3))
    n = len(V)
    out = {"metric": "points_orient", "reps": a.reps, "points": n, "k": a.k}

    tree = K.KdTree(V)
    h = tree.handle
    Vd = torch.from_numpy(V).to(dev)
    nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
    work = torch.empty_like(nrm)
    inf = float("inf")
    out["normals"] = timed(lambda: N.check(L.sdfk_points_normals_device(h, a.k, inf, None, 0, p(nrm), None)))
    st = (C.c_int64 * 9)()
    orient = timed(lambda: N.check(L.sdfk_points_orient_normals_device(h, a.k, inf, 64, p(work), st)), before=lambda: work.copy_(nrm))
    sync()
    outward = lambda t: round(float(((t * Vd).sum(dim=1) > 0).float().mean().item()), 6)
    orient.update(rounds=int(st[0]), seeds=int(st[1]), flipped=int(st[2]), unreached=int(st[3]), invalid=int(st[4]),
                  levels=[int(v) for v in st[5:9]], outward_before=outward(nrm), outward_after=outward(work),
                  ratio_to_normals=round(orient["ms"] / out["normals"]["ms"], 3))
    out["orient"] = orient
    N.check(L.sdfk_set_stream(None))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
