"""Rays against triangle meshes (MeshSdf.RayCast / Occluded / Render, csrc/lib_trimesh_ray.hip) on the MI355X: one JSON line, also
written to profiles/mesh_ray_bench.json.

  The clipped 512^3 marching-cubes mesh of Sdfs.Sphere(1) over -1.25..1.25 (1.58 M triangles), a handle made before the clock starts:
    render_depth / render_rgb   sdfk_trimesh_render_device, 1920 x 1080, the camera at (1.5, 0.9, 2.4) looking at the centre
    raycast / occluded          sdfk_trimesh_raycast_device, 2 M random rays from origins inside the ball of radius 0.5, first hit
                                with all three outputs, and the same rays with SDFK_RAY_ANY_HIT
    closest                     the yardstick that exists on this handle: sdfk_trimesh_closest_device on 2 M queries, the hit
                                points of those rays moved along the ray by up to four voxels either way (near the surface, where
                                the search is used: registration, banded volumes)
  Each figure is the median over --reps timed blocks, min and max as the spread; a block is --calls calls on device buffers ended
  by one device synchronise, host wall clock, after one warm-up block.  tests_per_ray is stats[5] / stats[6] of one further call
  under sdfk_profile_enable(1): the binary64 ray-triangle tests per ray, which does not depend on clocks and says how well the walk
  prunes (for closest: the binary64 closest-point evaluations per query).
  python tools/bench_mesh_ray.py [--reps 7] [--calls 4] [--n 512] [--rays 2000000]
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


def _blocks(fn, reps, calls, sync, items):
    for _ in range(calls):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3 / calls)
    ts.sort()
    med = ts[len(ts) // 2]
    return {"median_ms": round(med, 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "per_second": round(items / (med * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--n", type=int, default=512, help="the grid of the sphere mesh")
    ap.add_argument("--rays", type=int, default=2_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import torch
    import sdfkit_amd as K
    from sdfkit_amd import _native as N
    from sdfkit_amd.meshsdf import MeshSdf
    N.init()
    L = N.lib()
    sync = lambda: (L.sdfk_synchronize(), torch.cuda.synchronize())  # noqa: E731
    m = K.Sdfs.Sphere(1.0).ToMesh([-1.25] * 3, [1.25] * 3, args.n, args.n, args.n, clipToBounds=True)
    V, T = np.array(m.Vertices, f32), np.array(m.Triangles, np.int32)
    t = MeshSdf((V, T))
    dev = torch.device("cuda", N._inited_device or 0)
    st = t.stats()
    out = {"triangles": st["triangles"], "grid": list(st["grid"]), "triangle_cell_pairs": st["entries"], "reps": args.reps, "calls_per_block": args.calls}

    def tests_per(call):
        N.check(L.sdfk_profile_enable(1))
        call()
        sync()
        N.check(L.sdfk_profile_enable(0))
        s = t.stats()
        return round(s["candidates"] / max(s["queries"], 1), 3)

    # ---- the camera render
    w, h = args.width, args.height
    pos, vpi, near, far = MeshSdf._camera(w, h, ((1.5, 0.9, 2.4), (0, 0, 0), (0, 1, 0)), None, None, None)
    depth = torch.empty(w * h, dtype=torch.float32, device=dev)
    rgb = torch.empty((w * h, 3), dtype=torch.float32, device=dev)
    sync()
    for name, (dp, cp) in (("render_depth", (depth.data_ptr(), None)), ("render_rgb", (None, rgb.data_ptr()))):
        call = lambda: t.RenderDevice(w, h, pos, vpi, near, far, dp, cp, None)  # noqa: E731
        out[name] = _blocks(call, args.reps, args.calls, sync, w * h)
        out[name]["tests_per_ray"] = tests_per(call)
    out["render_depth"]["pixels"] = w * h
    out["render_depth"]["hit_fraction"] = round(float(torch.isfinite(depth).float().mean().item()), 4)

    # ---- random rays from inside
    n = args.rays
    rng = np.random.default_rng(1)
    D = rng.normal(size=(n, 3))
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(f32)
    O = rng.normal(size=(n, 3))
    O = (O / np.linalg.norm(O, axis=1, keepdims=True) * (0.5 * rng.uniform(0, 1, (n, 1)) ** (1 / 3))).astype(f32)
    o, d = torch.from_numpy(O).to(dev), torch.from_numpy(D).to(dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    wts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    sync()
    cast = lambda: t.RayCastDevice(o.data_ptr(), d.data_ptr(), n, 0.0, np.inf, tri.data_ptr(), dist.data_ptr(), wts.data_ptr())  # noqa: E731
    occ = lambda: t.RayCastDevice(o.data_ptr(), d.data_ptr(), n, 0.0, np.inf, tri.data_ptr(), None, None, anyHit=True)  # noqa: E731
    out["raycast"] = _blocks(cast, args.reps, args.calls, sync, n)
    out["raycast"]["tests_per_ray"] = tests_per(cast)
    cast()
    sync()
    out["raycast"]["hit_fraction"] = round(float((tri >= 0).float().mean().item()), 4)
    hit_t = dist.cpu().numpy()
    out["occluded"] = _blocks(occ, args.reps, args.calls, sync, n)
    out["occluded"]["tests_per_ray"] = tests_per(occ)

    # ---- the yardstick: closest triangle of as many queries near the surface
    voxel = 2.5 / args.n
    shift = rng.uniform(-4 * voxel, 4 * voxel, n).astype(f32)
    Q = (O + D * (np.where(np.isfinite(hit_t), hit_t, f32(1.0)) + shift)[:, None]).astype(f32)
    q = torch.from_numpy(Q).to(dev)
    cp3 = torch.empty((n, 3), dtype=torch.float32, device=dev)
    sync()
    closest = lambda: N.check(L.sdfk_trimesh_closest_device(t.handle, C.c_void_p(q.data_ptr()), n, C.c_void_p(tri.data_ptr()),  # noqa: E731
                                                            C.c_void_p(dist.data_ptr()), C.c_void_p(cp3.data_ptr())))
    out["closest"] = _blocks(closest, args.reps, args.calls, sync, n)
    out["closest"]["evaluations_per_query"] = tests_per(closest)
    out["raycast"]["times_closest"] = round(out["raycast"]["median_ms"] / out["closest"]["median_ms"], 2)
    out["occluded"]["times_closest"] = round(out["occluded"]["median_ms"] / out["closest"]["median_ms"], 2)
    out["rays"] = n
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_ray_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
