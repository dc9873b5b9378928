"""Depth fusion (DepthFusion.IntegrateDevice, DepthToPoints' device form; csrc/lib_fusion.hip) on the MI355X: one JSON line, also
written to profiles/depth_fusion_bench.json.

  Frames: the clipped 512^3 marching-cubes mesh of Sdfs.Sphere(1) over -1.25..1.25 (1.58 M triangles) rendered at 640 x 480 by
  sdfk_trimesh_render_device from 14 poses at distance 4 to 4.3 (before the clock starts; the frames stay in device memory).
  Volumes: 256^3 and 512^3 over the same box, truncation three voxels.
    integrate_carve / integrate_open   sdfk_volume_integrate_depth_device per frame, with SDFK_FUSE_CARVE_BEYOND (a frame updates all
                                       it sees in front of the surface) and without (the truncation band only), as ms per frame and
                                       as GB/s of the bytes a frame must move: 16 per updated voxel (D and W read and written)
    plain_pass                         the bound of a frame that sees everything: an in-place elementwise pass (torch's add_) over two
                                       f32 arrays of the volumes' size, reading and writing every byte, in the same process
    unproject                          sdfk_depth_unproject_device per frame, points and pixels (the count's read-back included)
  Library and torch share one stream (bind_torch_stream); a figure is the median over --reps blocks timed with device events on that
  stream, min and max as the spread, after one warm-up block; a block is one pass over the 14 frames.
  python tools/bench_depth_fusion.py [--reps 7] [--n 512] [--sizes 256 512]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

f32 = np.float32
VIEWS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] + [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]


def view(k):
    v = np.asarray(VIEWS[k], np.float64)
    pos = v / np.sqrt(v @ v) * (4.0 + 0.3 * k / (len(VIEWS) - 1))
    up = (0.0, 0.0, 1.0) if VIEWS[k][0] == 0 and VIEWS[k][2] == 0 else (0.0, 1.0, 0.0)
    return (tuple(float(x) for x in pos), (0.0, 0.0, 0.0), up)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=512, help="the grid of the sphere mesh")
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    args = ap.parse_args()
    import torch
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from sdfkit_amd.fusion import Camera, DepthFusion
    from sdfkit_amd.meshsdf import MeshSdf
    N.init()
    L = N.lib()
    stream = N.bind_torch_stream()
    dev = torch.device("cuda", N._inited_device or 0)
    w, h = args.width, args.height

    def timed(block, per):
        """median / min / max ms of block() / per over the repetitions, device events on the shared stream"""
        block()
        stream.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            block()
            b.record(stream)
            b.synchronize()
            ts.append(a.elapsed_time(b) / per)
        ts.sort()
        return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}

    m = K.Sdfs.Sphere(1.0).ToMesh([-1.25] * 3, [1.25] * 3, args.n, args.n, args.n, clipToBounds=True)
    t = MeshSdf((np.array(m.Vertices, f32), np.array(m.Triangles, np.int32)))
    cams, frames = [], []
    for k in range(len(VIEWS)):
        pos, vp, vpi, near, far = Camera(w, h, view(k))
        d = torch.empty(w * h, dtype=torch.float32, device=dev)
        t.RenderDevice(w, h, pos, vpi, near, far, d.data_ptr(), None, None)
        cams.append((pos, vp, vpi, near, far))
        frames.append(d)
    stream.synchronize()
    out = {"triangles": t.stats()["triangles"], "frames": len(frames), "width": w, "height": h, "reps": args.reps,
           "hit_fraction": round(float(torch.isfinite(torch.stack(frames)).float().mean().item()), 4), "volumes": {}}

    for n in args.sizes:
        voxel = 2.5 / n
        res = {"voxels": n ** 3, "truncation_voxels": 3}
        for label, carve in (("integrate_carve", True), ("integrate_open", False)):
            fu = DepthFusion([-1.25] * 3, [1.25] * 3, n, n, n, 3 * voxel, carve=carve)

            def block():
                for (pos, vp, _, near, far), d in zip(cams, frames):
                    fu.IntegrateDevice(d.data_ptr(), w, h, pos, vp, near, far)
            r = timed(block, len(frames))
            updated = []
            for (pos, vp, _, near, far), d in zip(cams, frames):   # (untimed: reading the counts synchronises)
                st = {}
                fu.IntegrateDevice(d.data_ptr(), w, h, pos, vp, near, far, stats=st)
                updated.append(st["updated"])
            mean_updated = float(np.mean(updated))
            r["updated_fraction"] = round(mean_updated / n ** 3, 4)
            r["needed_bytes_per_frame"] = int(16 * mean_updated)
            r["needed_GBps"] = round(16 * mean_updated / (r["median_ms"] * 1e-3) / 1e9, 1)
            res[label] = r
            del fu
        a = torch.zeros(n ** 3, dtype=torch.float32, device=dev)
        b = torch.zeros(n ** 3, dtype=torch.float32, device=dev)

        def plain():
            for _ in range(len(frames)):
                a.add_(1.0)
                b.add_(1.0)
        p = timed(plain, len(frames))
        p["bytes"] = 16 * n ** 3
        p["GBps"] = round(16 * n ** 3 / (p["median_ms"] * 1e-3) / 1e9, 1)
        res["plain_pass"] = p
        for label in ("integrate_carve", "integrate_open"):
            res[label]["times_plain_pass"] = round(res[label]["median_ms"] / p["median_ms"], 3)
        del a, b
        out["volumes"][str(n)] = res

    # ---- a frame as points
    pts = torch.empty((w * h, 3), dtype=torch.float32, device=dev)
    pix = torch.empty(w * h, dtype=torch.int32, device=dev)
    count = C.c_int64()
    m16 = lambda x: (C.c_float * 16)(*[float(v) for v in np.asarray(x, f32).ravel()])  # noqa: E731
    valid = []

    def unproject():
        valid.clear()
        for (pos, _, vpi, near, far), d in zip(cams, frames):
            N.check(L.sdfk_depth_unproject_device(C.c_void_p(d.data_ptr()), None, w, h, N.f3(pos), m16(vpi), C.c_float(near), C.c_float(far),
                                                  C.c_void_p(pts.data_ptr()), None, C.c_void_p(pix.data_ptr()), C.byref(count)))
            valid.append(count.value)
    out["unproject"] = timed(unproject, len(frames))
    out["unproject"]["points_per_frame"] = int(np.mean(valid))
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "depth_fusion_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
