"""KdTree.VoxelDownsample and RemoveStatisticalOutliers on the MI355X: one JSON line (kept as profiles/points_filter_bench.json).

  mesh:    the 549 144 vertices of the 512^3 sphere mesh (Sdfs.Sphere(1), bounds -1.5..1.5, no clip) concatenated with a copy moved
           by a quarter of a voxel -- two scans of one surface -- downsampled at a voxel size of two voxels of the mesh's grid, and
           filtered at k = 8, stdRatio = 2
  uniform: 10^7 uniform points in [0, 1)^3 at a voxel size of 0.01 (about 10^6 voxels), and the same outlier filter
  numpy:   the same filters on the host: np.floor + np.unique + np.add.at for the downsample; scipy.spatial.cKDTree.query(k = 9,
           workers = 16) + mean / std for the outliers (left out without scipy)
  sort:    torch.sort of the same packed 64-bit voxel keys on the same device (stable = True), the yardstick of the hand-written
           radix sort; the library's own sort time and its passes come from its profile spans (k_rs_pass: one span per pass)

Every leg: the median of --reps host wall-clock times around a call that has finished when it returns, with min..max; device
buffers are torch tensors, so host copies are excluded.  phases_ms: the library's profile spans of one more call under
sdfk_profile_enable(1).  Kernel times come from a rocprofv3 --kernel-trace --stats run of this script (--skip-cpu --skip-uniform).
  python tools/bench_points_filter.py [--reps 5] [--skip-cpu] [--skip-uniform]
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

    def phases(fn):
        N.check(L.sdfk_profile_reset())
        N.check(L.sdfk_profile_enable(1))
        fn()
        sync()
        snap = N.profile_snapshot()
        N.check(L.sdfk_profile_enable(0))
        return {k: {"ms": round(v[0], 4), "spans": int(v[1])} for k, v in snap.items() if k.startswith(("k_vf_", "k_rs_", "k_of_"))}

    def leg(P, size, k, ratio, cpu):
        n = len(P)
        Pd = torch.from_numpy(P).to(dev)
        h = C.c_void_p()
        N.check(L.sdfk_points_create_device(p(Pd), n, C.byref(h)))
        pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        grp = torch.empty(n, dtype=torch.int32, device=dev)
        m = C.c_int64()
        origin = (C.c_float * 3)(0.0, 0.0, 0.0)

        def down():
            N.check(L.sdfk_points_voxel_downsample_device(h, float(size), origin, p(pts), p(cnt), p(grp), C.byref(m)))
        res = {"points": n, "voxel_size": round(float(size), 6), "downsample": timed(down)}
        res["downsample"].update(voxels=int(m.value), phases_ms=phases(down))
        sort = res["downsample"]["phases_ms"].get("k_rs_pass", {"ms": 0.0, "spans": 0})
        # the yardstick of the sort: torch.sort of the same keys
        lo = P.min(axis=0)
        kk = np.floor(P.astype(np.float64) / np.float64(f32(size)))
        kk = (kk - kk.min(axis=0)).astype(np.int64)
        keys = torch.from_numpy(kk[:, 2] << 42 | kk[:, 1] << 21 | kk[:, 0]).to(dev)
        ts = timed(lambda: torch.sort(keys, stable=True))
        res["sort"] = {"radix_ms": sort["ms"], "radix_passes": sort["spans"], "radix_ms_per_pass": round(sort["ms"] / max(1, sort["spans"]), 4),
                       "torch_sort_ms": ts["ms"], "ratio_to_torch_sort": round(sort["ms"] / ts["ms"], 3)}
        del keys, lo
        mean = torch.empty(n, dtype=torch.float32, device=dev)
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        kept = C.c_int64()
        st = (C.c_int64 * 6)()

        def out():
            N.check(L.sdfk_points_outliers_device(h, k, ratio, float("inf"), p(mean), p(keep), p(cnt), p(pts), C.byref(kept), st))
        res["outliers"] = timed(out)
        res["outliers"].update(k=k, std_ratio=ratio, kept=int(st[0]), removed=int(st[1]), isolated=int(st[2]), phases_ms=phases(out))
        L.sdfk_points_free(h)
        if cpu:
            t0 = time.perf_counter()
            uniq, inv = np.unique(kk[:, 2] << 42 | kk[:, 1] << 21 | kk[:, 0], return_inverse=True)
            sums = np.zeros((len(uniq), 3))
            np.add.at(sums, inv, P)
            cent = sums / np.bincount(inv)[:, None]
            res["cpu_numpy"] = {"downsample_ms": round(1e3 * (time.perf_counter() - t0), 2), "voxels": len(cent)}
            try:
                from scipy.spatial import cKDTree
                t0 = time.perf_counter()
                d, _ = cKDTree(P).query(P, k=k + 1, workers=16)
                md = d[:, 1:].mean(axis=1)
                keep_cpu = md <= md.mean() + ratio * md.std()
                res["cpu_numpy"].update(outliers_ckdtree_16w_ms=round(1e3 * (time.perf_counter() - t0), 2), kept=int(keep_cpu.sum()))
            except ImportError:
                pass
        return res

    out = {"metric": "points_filter", "reps": a.reps}
    n = a.n
    mesh = K.Sdfs.Sphere(1.0).ToMesh([-1.5] * 3, [1.5] * 3, n, n, n, clipToBounds=False)
    V = np.ascontiguousarray(np.asarray(mesh.Vertices, f32).reshape(-1, 3))
    spacing = 3.0 / (n - 1)
    merged = np.concatenate([V, (V + f32(0.25 * spacing)).astype(f32)])
    out["mesh"] = leg(merged, f32(2.0 * spacing), 8, 2.0, not a.skip_cpu)
    if not a.skip_uniform:
        rs = np.random.default_rng(0)
        out["uniform"] = leg(rs.random((10_000_000, 3), dtype=f32), f32(0.01), 8, 2.0, not a.skip_cpu)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
