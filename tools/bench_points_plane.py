"""IterativeClosestPoint on the MI355X, point to plane against point to point on the same clouds: one JSON line.

  small: the height-field case of tests/icp_plane_model.py -- a 48 x 48 static grid with analytic normals, 700 off-grid points
  large: the same surface sampled 1024 x 1024 (1 048 576 static points), 262 144 off-grid dynamic points, the same motion

Per case and metric: iterations, the RMS distance to the true positions, and the host wall clock of RegisterDevicePoints (ends in
a device synchronise; median of --reps after one warm-up; points and normals are torch tensors, so host copies are excluded).
Kernel times come from a rocprofv3 --kernel-trace --stats run of this script.
  python tools/bench_points_plane.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    import torch
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from tests import icp_plane_model as M

    N.init(0)
    L = N.lib()
    N.bind_torch_stream()
    dev = torch.device("cuda:0")

    def sync():
        N.check(L.sdfk_synchronize())

    out = {"bench": "points_plane", "reps": a.reps}
    for name, m, n in (("small", 48, 700), ("large", 1024, 1 << 18)):
        S, Nn = M.height_field_static(m)
        D0, D = M.height_field_dynamic(n)
        icp = K.IterativeClosestPoint(S)
        nrm = torch.from_numpy(Nn).to(dev)
        src = torch.from_numpy(D).to(dev)
        torch.cuda.synchronize()
        case = {"static": len(S), "dynamic": n}
        for metric in ("point", "plane"):
            icp.StaticNormals = Nn if metric == "plane" else None
            ts = []
            for rep in range(a.reps + 1):
                pts = src.clone()
                torch.cuda.synchronize()
                sync()
                t0 = time.perf_counter()
                icp.RegisterDevicePoints(pts.data_ptr(), n, normals_dev=nrm.data_ptr() if metric == "plane" else None)
                sync()
                ts.append(1e3 * (time.perf_counter() - t0))
            ts = ts[1:]
            case[metric] = {"iterations": icp.Iterations, "rms": M.rms(pts.cpu().numpy(), D0), "call_ms": round(float(np.median(ts)), 4),
                            "ms_per_iteration": round(float(np.median(ts)) / max(1, icp.Iterations), 4), "call_ms_all": [round(t, 4) for t in ts]}
            if metric == "plane":
                case[metric]["stats"] = {k: v for k, v in icp.LastStats.items() if k != "raw"}
        out[name] = case
    print(json.dumps(out))


if __name__ == "__main__":
    main()
