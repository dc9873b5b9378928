"""Mesh sampling (MeshSdf.SamplePoints, csrc/lib_trimesh.hip: k_tm_area2, k_tm_sample_weights, the scan, k_tm_sample) on the
MI355X: one JSON line.

  mesh:   the clipped 512^3 mesh of Sdfs.Sphere(1) over -1.25..1.25 (1.58 M triangles), with a colour per vertex
  first:  the first sampling call of a fresh handle (weights + scan + the synchronise that reads the total + 10^6 samples)
  sample: 10^6 and 10^7 samples, plain and stratified, sdfk_trimesh_sample_device into preallocated device buffers with all five
          outputs requested (52 bytes written per sample)
Times are host wall clock around work that ends in a device synchronise (median of --reps after one warm-up call of the same
shape, min and max given as the spread).  write_fraction_of_peak: the 52 n bytes a call must write over its median time, as a
fraction of the 8 TB/s peak of the HBM: a whole-call figure (launch and synchronise included), not a kernel's share of peak; the
reads (the search over W, the 64-byte triangle and three colour gathers) come on top.  Kernel times come from a rocprofv3
--kernel-trace --stats run of this script.
  python tools/bench_mesh_sample.py [--reps 5] [--n 512]
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
BYTES_PER_SAMPLE = 52          # points, normals, colours, weights (12 each) + the triangle index (4)
PEAK_BYTES_PER_S = 8e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=512, help="the grid of the sphere mesh")
    args = ap.parse_args()
    import torch
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from sdfkit_amd.meshsdf import MeshSdf
    N.init()
    L = N.lib()
    sync = lambda: (L.sdfk_synchronize(), torch.cuda.synchronize())  # noqa: E731
    out = {}
    m = K.Sdfs.Sphere(1.0).ToMesh([-1.25] * 3, [1.25] * 3, args.n, args.n, args.n, clipToBounds=True)
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, np.int32)
    cols = (0.5 + 0.4 * V).astype(f32)
    out["triangles"] = len(T) // 3
    big = 10_000_000
    dev = torch.device("cuda", N._inited_device or 0)
    bufs = [torch.empty((big, 3), dtype=torch.float32, device=dev) for _ in range(3)] + [torch.empty(big, dtype=torch.int32, device=dev),
                                                                                        torch.empty((big, 3), dtype=torch.float32, device=dev)]
    ptrs = [b.data_ptr() for b in bufs]
    torch.cuda.synchronize()
    handles = [MeshSdf((V, T, cols)) for _ in range(args.reps + 1)]
    fresh = iter(handles)
    # (each repetition takes a handle that has not sampled yet; the warm-up of the shape is the first of them)
    out["first_call_1e6"] = _times(lambda: next(fresh).SamplePointsDevice(1_000_000, 1, True, *ptrs), args.reps, sync)
    t = handles[0]
    out["stats"] = t.sample_stats()
    for n, tag in ((1_000_000, "1e6"), (big, "1e7")):
        for strat in (False, True):
            r = _times(lambda: t.SamplePointsDevice(n, 1, strat, *ptrs), args.reps, sync)
            r["write_fraction_of_peak"] = round(BYTES_PER_SAMPLE * n / (r["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
            out[f"sample_{tag}_{'stratified' if strat else 'plain'}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
