"""KdTree.Clusters on the MI355X: one JSON line (kept as profiles/points_cluster_bench.json).

  cloud:   the cloud of tools/bench_pointcloud.py: the 549 144 vertices of the 512^3 sphere mesh (Sdfs.Sphere(1), bounds -1.5..1.5,
           no clip); radius = three spacings of the mesh's grid
  cluster: sdfk_points_cluster_device at min_points = 1 (Euclidean clustering) and 8, every output asked for: the whole call, its
           hook rounds and shortcut launches, clusters / core / border / noise
  floor:   one sdfk_points_radius_count_device call over the same points and radius in the same run -- a single walk, which the
           count kernel, every hook round and the border kernel each repeat: walks = the whole call over the floor, next to the
           2 + rounds that it is expected to cost
  select:  sdfk_points_select_device keeping the largest cluster

Every leg: the median of --reps host wall-clock times around a call that has finished when it returns (the floor: that ends in a
device synchronise), warmed, with min..max; device buffers are torch tensors, so host copies are excluded.  phases_ms: the library's
profile spans of one more call under sdfk_profile_enable(1) (which synchronises after every walk).
  python tools/bench_points_cluster.py [--reps 5] [--n 512] [--spacings 3]
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
    ap.add_argument("--spacings", type=float, default=3.0, help="the radius in spacings of that grid")
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

    def phases(fn):
        N.check(L.sdfk_profile_reset())
        N.check(L.sdfk_profile_enable(1))
        fn()
        sync()
        snap = N.profile_snapshot()
        N.check(L.sdfk_profile_enable(0))
        return {k: {"ms": round(v[0], 4), "spans": int(v[1])} for k, v in snap.items() if k.startswith(("k_cl_", "k_cs_"))}

    mesh = K.Sdfs.Sphere(1.0).ToMesh([-1.5] * 3, [1.5] * 3, a.n, a.n, a.n, clipToBounds=False)
    V = np.ascontiguousarray(np.asarray(mesh.Vertices, f32).reshape(-1, 3))
    n = len(V)
    radius = float(f32(a.spacings * 3.0 / (a.n - 1)))
    Pd = torch.from_numpy(V).to(dev)
    h = C.c_void_p()
    N.check(L.sdfk_points_create_device(p(Pd), n, C.byref(h)))
    out = {"metric": "points_cluster", "reps": a.reps, "points": n, "radius": round(radius, 6), "radius_spacings": a.spacings}

    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    out["floor_radius_count"] = timed(lambda: N.check(L.sdfk_points_radius_count_device(h, p(Pd), n, radius, p(off))))
    sync()
    out["floor_radius_count"]["mean_neighbours"] = round(int(off[n].item()) / n, 2)
    floor = out["floor_radius_count"]["ms"]

    labels = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    core = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    c = C.c_int64()
    st = (C.c_int64 * 6)()
    for mp in (1, 8):
        def run():
            N.check(L.sdfk_points_cluster_device(h, radius, mp, p(labels), p(sizes), p(core), p(counts), C.byref(c), st))
        leg = timed(run)
        leg.update(min_points=mp, clusters=int(st[0]), core=int(st[1]), border=int(st[2]), noise=int(st[3]), hook_rounds=int(st[4]),
                   shortcut_launches=int(st[5]), walks_expected=2 + int(st[4]), walks_measured=round(leg["ms"] / floor, 2), phases_ms=phases(run))
        out[f"cluster_min_points_{mp}"] = leg

    C_ = int(c.value)
    keep = torch.zeros(max(1, C_), dtype=torch.uint8, device=dev)
    if C_:
        keep[int(torch.argmax(sizes[:C_]).item())] = 1
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    kept = C.c_int64()
    out["select_largest"] = timed(lambda: N.check(L.sdfk_points_select_device(h, p(labels), p(keep), C_, p(idx), p(pts), C.byref(kept))))
    out["select_largest"]["kept"] = int(kept.value)
    L.sdfk_points_free(h)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
