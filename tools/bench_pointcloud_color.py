"""Per-point colours in the point-cloud pipeline on the MI355X: one JSON line (kept as profiles/pointcloud_color_bench.json).

  cloud:    the 549 144 vertices of the 512^3 sphere mesh (Sdfs.Sphere(1), bounds -1.5..1.5, no clip), their mesh normals,
            colours 0.5 + 0.25 p -- the shapes of tools/bench_pointcloud.py
  volume:   sdfk_points_to_volume_colors_device into 256^3 with a band of 4 voxels at k = 8 and 16, against
            sdfk_points_to_volume_device alone with the same arguments, the two alternating in the same run: ratio_to_plain
  sample:   sdfk_points_blend_colors_device at k = 8 and 16 on the cloud's own points, against sdfk_points_knn_device at the same
            k on the same queries, writing its whole rows (what SearchKNearest returns) and writing `found` only: ratio_to_knn
            is to the whole rows

Every leg: the median of --reps host wall-clock times around a call that ends in a device synchronise, with min..max.
  python tools/bench_pointcloud_color.py [--reps 7] [--n 512] [--grid 256]
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
    ap.add_argument("--reps", type=int, default=7)
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

    def timed_together(fns):
        """The legs of `fns` (name -> call) alternating, so that what else the machine does meets all of them alike."""
        for fn in fns.values():
            fn()   # warm-up
        ts = {name: [] for name in fns}
        for _ in range(a.reps):
            for name, fn in fns.items():
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                ts[name].append(1e3 * (time.perf_counter() - t0))
        return {name: {"ms": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for name, v in ts.items()}

    mesh = K.Sdfs.Sphere(1.0).ToMesh([-1.5] * 3, [1.5] * 3, a.n, a.n, a.n, clipToBounds=False)
    V = np.ascontiguousarray(np.asarray(mesh.Vertices, f32).reshape(-1, 3))
    Nm = np.ascontiguousarray(np.asarray(mesh.Normals, f32).reshape(-1, 3))
    col = (f32(0.5) + f32(0.25) * V).astype(f32)
    n = len(V)
    g = a.grid
    band = 4 * 3.0 / g
    out = {"metric": "pointcloud_color", "reps": a.reps, "points": n, "grid": g, "band_voxels": 4}

    tree = K.KdTree(V)
    h = tree.handle
    Vd, Nd, Cd = (torch.from_numpy(x).to(dev) for x in (V, Nm, col))

    plain_vox = K.Voxels([-1.5] * 3, [1.5] * 3, g, g, g)
    color_vox = K.Voxels([-1.5] * 3, [1.5] * 3, g, g, g)
    hp, hc = plain_vox._ensure_device(False), color_vox._ensure_device(True)
    st = (C.c_int64 * 4)()
    for k in (8, 16):
        r = timed_together({
            "plain": lambda: N.check(L.sdfk_points_to_volume_device(h, p(Nd), hp, k, band, None)),
            "colors": lambda: N.check(L.sdfk_points_to_volume_colors_device(h, p(Nd), p(Cd), hc, k, band, None)),
        })
        N.check(L.sdfk_points_to_volume_colors_device(h, p(Nd), p(Cd), hc, k, band, st))
        leg = r["colors"]
        leg.update(plain_ms=r["plain"]["ms"], plain_ms_min=r["plain"]["ms_min"], plain_ms_max=r["plain"]["ms_max"],
                   ratio_to_plain=round(leg["ms"] / r["plain"]["ms"], 3), known=int(st[0]), unknown=int(st[1]))
        out[f"volume_{k}"] = leg

    found = torch.empty(n, dtype=torch.int32, device=dev)
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    for k in (8, 16):
        idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        dist = torch.empty((n, k), dtype=torch.float32, device=dev)
        r = timed_together({
            "knn_rows": lambda: N.check(L.sdfk_points_knn_device(h, p(Vd), n, k, float("inf"), p(idx), p(dist), p(found))),
            "knn_found": lambda: N.check(L.sdfk_points_knn_device(h, p(Vd), n, k, float("inf"), None, None, p(found))),
            "colors": lambda: N.check(L.sdfk_points_blend_colors_device(h, p(Cd), p(Vd), n, k, float("inf"), p(rgb), p(found))),
        })
        leg = r["colors"]
        leg.update(knn_ms=r["knn_rows"]["ms"], knn_found_only_ms=r["knn_found"]["ms"], ratio_to_knn=round(leg["ms"] / r["knn_rows"]["ms"], 3),
                   ratio_to_knn_found_only=round(leg["ms"] / r["knn_found"]["ms"], 3))
        out[f"sample_{k}"] = leg
    N.check(L.sdfk_set_stream(None))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
