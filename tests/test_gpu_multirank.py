"""The multi-rank path end to end on ONE GPU.  `bench.py --gpus N` under torch.distributed.run with
SDFK_BENCH_ONE_GPU=1: every rank on GPU 0, the exchange through the library's HOST transport (a gloo all-gather;
RCCL refuses two ranks on one device).  Everything else is the production code behind the C ABI (sdfk_dist_*): Z-slab
partition, speculative slab steps on the library's lanes emitted straight into the gather buffer, the C++ step
protocol, rebase, header mirror, mesh extraction.  Real RCCL is exercised at world = 1."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bench(extra, env=None):
    e = dict(os.environ)
    e.update(env or {})
    out = subprocess.run(extra, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(lines[-1])


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_bench_on_one_gpu(gpu, world):
    args = ["--full", "--steps", "6", "--warmup", "2", "--no-cpu", "--scene", "repeatxy", "--grid", "160"]
    one = _bench([sys.executable, "bench.py"] + args)
    many = _bench([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                   "--master-port", str(_free_port()), "bench.py", "--gpus", str(world)] + args,
                  {"SDFK_BENCH_ONE_GPU": "1", "SDFK_BENCH_C4_GRID": "96", "SDFK_BENCH_C4_STEPS": "4"})
    assert many["n_gpus"] == world and one["n_gpus"] == 1
    assert many["config"]["vertices"] == one["config"]["vertices"] > 10000
    assert many["config"]["triangles"] == one["config"]["triangles"]
    for d in (one, many):
        for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype", "data", "config"):
            assert k in d
    assert one["roofline"]["bound"] == "hbm" and 0 < one["roofline"]["frac"] < 1.2
    # the pass that leaves the mesh sharded (exchange mode 3: only headers travel) ran after the headline and saw the same mesh
    p3 = many["sharded"]["mesh_stays_sharded_pass"]
    assert isinstance(p3, dict) and p3.get("counts_equal_the_headline_mesh") is True and p3["ms_per_step"] > 0, p3
    assert many["sharded"]["speedup_ceiling_mesh_stays_sharded"] is None or many["sharded"]["speedup_ceiling_mesh_stays_sharded"] > 0
    # CONTENT, not just counts: rank 0 meshed the same grid on one GPU and compared SHA-256 digests of the four arrays with the gathered
    # mesh -- for the headline, for the pass that leaves the mesh sharded (payloads gathered on demand) -- and every rank's own slab
    # with its slice
    sh = many["sharded"]
    assert sh["mesh_equals_single_gpu"] is True and sh["content_check"]["every_ranks_slab_equals_its_slice"] is True, sh["content_check"]
    assert sh["content_check"]["vertices"] == many["config"]["vertices"] and len(sh["content_check"]["sha256_single_gpu"]["Triangles"]) == 64
    assert p3["mesh_equals_single_gpu"] is True and p3["content_check"]["every_ranks_slab_equals_its_slice"] is True, p3
    # BASELINE config C4 (union of 8 primitives; here on a reduced grid) sharded in the same run, with the default exchange and with
    # the mesh left sharded: times, what every rank receives, the single-GPU step of the same grid, and the same content check
    c4 = sh["c4_union8_1024"]
    assert isinstance(c4, dict) and c4["grid"] == 96, c4
    for key, per_rank_bytes in (("all_gather", None), ("mesh_stays_sharded", (world - 1) * 64)):
        leg = c4[key]
        assert isinstance(leg, dict) and leg["ms_per_step"] > 0 and leg["steps"] == 4 and leg["vertices"] > 1000, leg
        assert leg["mesh_equals_single_gpu"] is True and leg["content_check"]["every_ranks_slab_equals_its_slice"] is True, leg
        assert leg["steps_redone"] == 0 and len(leg["per_rank_vertices_indices"]) == world
        # (the "all_gather" leg runs with the process's DEFAULT exchange: headers only when the suite runs under SDFK_DIST_EXCHANGE=3)
        if per_rank_bytes is None and os.environ.get("SDFK_DIST_EXCHANGE") == "3":
            per_rank_bytes = (world - 1) * 64
        assert leg["bytes_received_per_rank"] == (per_rank_bytes if per_rank_bytes is not None else (world - 1) * leg["gather_stride_bytes_per_rank"])
        assert leg["single_gpu_ms_per_step"] > 0 and leg["speedup_measured"] > 0 and leg["single_gpu_product_default_ms_per_step"] > 0
    assert c4["all_gather"]["vertices"] == c4["mesh_stays_sharded"]["vertices"]
    assert sh["every_mesh_equals_single_gpu"] is True and all(v is True for v in sh["content_checks"].values()), sh["content_checks"]
    assert {"headline", "mesh_stays_sharded_pass", "c4_all_gather", "c4_mesh_stays_sharded"} <= set(sh["content_checks"])
    assert one["blocks"]["n"] >= 1 and one["blocks"]["ms_per_step_min"] <= one["ms_per_step"] <= one["blocks"]["ms_per_step_max"]


def test_a_flipped_index_turns_the_content_check_false_and_fails_the_run(gpu):
    """Fault injection for the check itself: SDFK_BENCH_FAULT_FLIP_INDEX=1 flips ONE index of the gathered mesh on rank 0 before it is
    hashed.  The line must say `mesh_equals_single_gpu: false` and the run must exit non-zero (4) -- on a node of real GPUs that is what
    a wrong exchange or a wrong rebase would look like."""
    args = ["--full", "--steps", "4", "--warmup", "1", "--no-cpu", "--grid", "96"]
    e = dict(os.environ)
    e.update({"SDFK_BENCH_ONE_GPU": "1", "SDFK_BENCH_FAULT_FLIP_INDEX": "1", "SDFK_BENCH_C4_GRID": "64", "SDFK_BENCH_C4_STEPS": "2"})
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(_free_port()), "bench.py", "--gpus", "2"] + args, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode != 0 and len(lines) == 1, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    sh = json.loads(lines[0])["sharded"]
    assert sh["mesh_equals_single_gpu"] is False and sh["every_mesh_equals_single_gpu"] is False
    assert sh["content_check"]["sha256_sharded"] != "identical" and sh["content_check"]["sha256_sharded"]["Triangles"] != sh["content_check"]["sha256_single_gpu"]["Triangles"]
    assert sh["content_check"]["sha256_sharded"]["Vertices"] == sh["content_check"]["sha256_single_gpu"]["Vertices"]      # only the flipped array differs
    assert sh["content_check"]["every_ranks_slab_equals_its_slice"] is True          # (the slabs themselves were right: the fault is in the gathered copy)
    assert "DIFFERS from the single-GPU mesh" in out.stderr


@pytest.mark.parametrize("world", [2])
def test_bench_gpus_n_started_as_plain_python(gpu, world):
    """The way the driver starts the multi-GPU leg: `python bench.py --gpus N`, no launcher, no WORLD_SIZE.
    bench.py must spawn torch.distributed.run itself (as a child, before touching the GPU) and relay rank 0's line."""
    args = ["--full", "--steps", "6", "--warmup", "2", "--no-cpu", "--grid", "128"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SDFK_BENCH_ONE_GPU"] = "1"
    env.update({"SDFK_BENCH_C4_GRID": "64", "SDFK_BENCH_C4_STEPS": "2"})
    out = subprocess.run([sys.executable, "bench.py", "--gpus", str(world)] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    many = json.loads(lines[0])
    one = _bench([sys.executable, "bench.py"] + args)
    assert many["n_gpus"] == world and one["n_gpus"] == 1
    assert many["config"]["vertices"] == one["config"]["vertices"] > 10000
    assert many["config"]["triangles"] == one["config"]["triangles"]
    sh = many["sharded"]
    assert sh["world"] == world and len(sh["per_rank_vertices_indices"]) == world
    assert sum(p[0] for p in sh["per_rank_vertices_indices"]) == many["config"]["vertices"]
    assert sh["gather_bytes_received_per_rank"] == (world - 1) * sh["gather_stride_bytes_per_rank"]
    assert 0 < sh["slab_kernels_only_ms"] and sh["xgmi"]["receive_bound_ms"] > 0
    for k in ("latency_ms_single_stream", "first_call_ms", "first_call", "value_is", "pipeline_frac_is"):
        assert k in one
    # (one call at a time is not faster than the pipelined steady state -- with the lanes off, SDFK_LANES=0, the two are the same
    # thing measured twice, hence the slack)
    assert one["latency_ms_single_stream"] >= one["ms_per_step"] * 0.5


def _gpu_count():
    import torch
    return torch.cuda.device_count()   # (counting devices does not initialise the GPU in this process)


@pytest.mark.parametrize("exchange,index16", [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1)])
def test_two_gpus_real_rccl_parity(gpu, exchange, index16):
    """FIRST CONTACT between two GPUs, as a test: one rank per GPU, the library's own RCCL communicator, every exchange
    (ncclAllGather, grouped ncclSend / ncclRecv, gather-to-root) and both payload forms; every step's whole mesh must be the
    oracle's.  Skipped on a one-GPU box (the development boxes): there real RCCL runs at world 1 only
    (test_rccl_world_one_through_the_c_abi) and 2-4 ranks go through the host transport."""
    if _gpu_count() < 2:
        pytest.skip("needs two GPUs")
    env = dict(os.environ)
    env.update({"SDFK_TEST_REAL_RCCL": "1", "SDFK_DIST_EXCHANGE": str(exchange), "SDFK_DIST_INDEX16": str(index16),
                "HSA_ENABLE_IPC_MODE_LEGACY": "0", "NCCL_SOCKET_IFNAME": "lo", "GLOO_SOCKET_IFNAME": "lo"})
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "multirank_worker.py"), "readme_repeat_xy", "72", "64", "80"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.count("identical") == 2, out.stdout[-3000:] + out.stderr[-4000:]


def test_rccl_world_one_through_the_c_abi(gpu):
    """The library's own step driver over REAL RCCL (sdfk_dist_unique_id / sdfk_dist_init / sdfk_dist_to_mesh /
    sdfk_dist_session_*), world = 1 -- the only world size RCCL accepts on a one-GPU box: communicator creation through
    dlopen'ed librccl, the exchange stream, all three exchange modes, rebase + header mirror, mesh extraction.  Every mesh
    is bit-identical to the oracle's, i.e. to sdf.ToMesh on one GPU.  Runs in a child process: the communicator and its
    stream live until the process ends."""
    code = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import numpy as np
from oracle import oracle as O
from sdfkit_amd import _native as N
from sdfkit_amd import dist as D
from tests import scenes as S
from tests.test_gpu_parity import assert_mesh_equal
N.init(0)
L = N.lib()
buf = (C.c_ubyte * 128)()
N.check(L.sdfk_dist_unique_id(buf))
N.check(L.sdfk_dist_init(1, 0, buf))
assert D.info() == (1, 0, 1)
import os
if "SDFK_DIST_EXCHANGE" not in os.environ and "SDFK_DIST_INDEX16" not in os.environ:
    assert N.get_option(N.OPT_DIST_EXCHANGE) == 0 and N.get_option(N.OPT_DIST_INDEX16) == 0    # the defaults: the plainest collective
for name, dims in (("readme_repeat_xy", (40, 36, 44)), ("sphere_w", (64, 64, 64))):
    scene, sdf = S.CATALOGUE[name]()
    mn, mx = [-2.8125] * 3, [2.8125] * 3
    ov, oc = O.sample(scene, mn, mx, *dims)
    O.clip_to_bounds(ov, mn, mx)
    om = O.march(ov, oc, mn, mx)
    assert_mesh_equal(D.sharded_to_mesh(sdf, mn, mx, *dims), om)
    assert_mesh_equal(sdf.ToMesh(mn, mx, *dims), om)
    # (exchange, payload form, internal streams, steps in flight): the default, the opt-ins, the CONSERVATIVE retry grades of
    # bench.py (one step in flight; no lanes at all) and the compact gather-to-root form (tools/gpu_alt_configs.sh)
    for mode, idx16, lanes, depth in ((0, 0, 3, 3), (1, 0, 3, 3), (2, 0, 3, 3), (1, 1, 3, 3), (0, 1, 3, 3), (0, 0, 3, 1), (0, 0, 0, 1), (2, 1, 3, 3), (2, 1, 0, 1), (3, 0, 3, 3), (3, 1, 3, 1)):
        N.set_option(N.OPT_DIST_EXCHANGE, mode)
        N.set_option(N.OPT_DIST_INDEX16, idx16)
        N.set_option(N.OPT_DIST_LANES, lanes)
        ses = D.SlabSession(sdf, mn, mx, *dims, True, 0.0, depth=depth)
        for it in range(12):
            if ses.in_flight == ses.depth:
                nv, ni = ses.collect()
                assert (nv, ni) == (len(om.vertices), len(om.triangles))
                if it %% 4 == 0:
                    assert_mesh_equal(ses.mesh(), om)
            ses.submit()
        ses.drain()
        assert_mesh_equal(ses.mesh(), om)
        st = ses.stats()
        assert st["steps"] == 12 and st["redone"] == 0 and st["exchange_mode"] == mode and st["index16"] == bool(idx16), st
        g, stride = C.c_void_p(), C.c_int64()
        N.check(L.sdfk_dist_gathered(ses.h, C.byref(g), C.byref(stride)))
        nv_, ni_ = len(om.vertices), len(om.triangles)
        vb = 36 if sdf.writes_color else 24
        need = 64 + vb * nv_ + (4 * ni_ if not idx16 else ((2 * ni_ + 3) & ~3) + 4 * ((ni_ + 1023) // 1024))
        assert g.value and stride.value == st["stride_bytes"] == (need + need // 32 + 4096 + 255) // 256 * 256   # (slab_protocol.h)
        ses.close()
    N.set_option(N.OPT_DIST_INDEX16, 0)
    N.set_option(N.OPT_DIST_LANES, 3)
    # the tuner: both exchanges x both payload forms, measured; whatever it keeps, the steps after it are the same mesh
    N.set_option(N.OPT_DIST_EXCHANGE, 1)
    for start16 in (0, 1):
        N.set_option(N.OPT_DIST_INDEX16, start16)
        ses = D.SlabSession(sdf, mn, mx, *dims, True, 0.0, depth=3)
        for it in range(4):
            ses.submit()
            ses.collect()
        t = ses.tune(6)
        assert set(t) == {(0, False), (1, False), (0, True), (1, True)} and all(v > 0 for v in t.values()), t
        st = ses.stats()
        best = min(t, key=lambda k: (t[k], k != (0, False)))
        assert (st["exchange_mode"], st["index16"]) == best, (st, t)
        for it in range(7):
            if ses.in_flight == ses.depth:
                assert ses.collect() == (len(om.vertices), len(om.triangles))
            ses.submit()
        ses.drain()
        assert_mesh_equal(ses.mesh(), om)
        assert ses.stats()["redone"] == 0 and ses.stats()["index16_fallbacks"] == 0
        ses.close()
    N.set_option(N.OPT_DIST_INDEX16, 0)
    # a session whose exchange mode is a CONTRACT (2: rank 0 holds the mesh, 3: the mesh stays sharded) is not the tuner's to change
    for mode in (2, 3):
        N.set_option(N.OPT_DIST_EXCHANGE, mode)
        ses = D.SlabSession(sdf, mn, mx, *dims, True, 0.0, depth=2)
        ses.submit()
        ses.collect()
        try:
            ses.tune(4)
            raise SystemExit("sdfk_dist_tune accepted exchange mode %%d" %% mode)
        except N.SdfKitNativeError as e:
            assert e.status == N.ERR_UNSUPPORTED and "contract" in str(e), e
        assert ses.stats()["exchange_mode"] == mode
        ses.submit()
        ses.collect()
        assert_mesh_equal(ses.mesh(), om)
        ses.close()
    N.set_option(N.OPT_DIST_EXCHANGE, 0)
D.shutdown()
print("rccl world 1 ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "rccl world 1 ok" in out.stdout, out.stdout[-3000:] + out.stderr[-4000:]


def test_index16_falls_back_when_a_slab_does_not_fit(gpu):
    """A tilted plane through a 512 x 512 x 8 grid: it crosses every layer over a third of the x extent, ~100 k active cells per
    layer, so triangles that reference the layer below reach back far more than 65535 vertex ids.  With SDFK_OPT_DIST_INDEX16 the compact encoder flags it in the payload header, every rank
    (one here) sees the flag, the session goes back to int32 indices, redoes the step exactly and regrows its buffers; the
    meshes are the oracle's throughout.  Child process (an RCCL communicator lives until the process ends)."""
    code = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import numpy as np
from oracle import oracle as O
from sdfkit_amd import _native as N
from sdfkit_amd import dist as D
from tests import scenes as S
from tests.test_gpu_parity import assert_mesh_equal
N.init(0)
L = N.lib()
buf = (C.c_ubyte * 128)()
N.check(L.sdfk_dist_unique_id(buf))
N.check(L.sdfk_dist_init(1, 0, buf))
scene, sdf = S.plane_w((0.3, 0.0, 1.0), 0.05)
mn, mx, dims = [-2.0] * 3, [2.0] * 3, (512, 512, 8)
ov, oc = O.sample(scene, mn, mx, *dims)
om = O.march(ov, oc, mn, mx)
assert len(om.vertices) > 200000
N.set_option(N.OPT_DIST_INDEX16, 1)
ses = D.SlabSession(sdf, mn, mx, *dims, False, 0.0, depth=2)
for it in range(7):
    if ses.in_flight == ses.depth:
        ses.collect()
        assert_mesh_equal(ses.mesh(), om)
    ses.submit()
ses.drain()
assert_mesh_equal(ses.mesh(), om)
st = ses.stats()
assert not st["index16"] and st["index16_fallbacks"] == 1 and st["regrown"] >= 1, st   # (found by the bootstrap step itself: done again with int32 indices)
ses.close()
# a scene that does fit stays compact
scene, sdf = S.sphere_w(1.0)
mn, mx, dims = [-1.5] * 3, [1.5] * 3, (96, 96, 96)
ov, oc = O.sample(scene, mn, mx, *dims)
om = O.march(ov, oc, mn, mx)
ses = D.SlabSession(sdf, mn, mx, *dims, False, 0.0, depth=2)
for it in range(6):
    if ses.in_flight == ses.depth:
        ses.collect()
    ses.submit()
ses.drain()
assert_mesh_equal(ses.mesh(), om)
st = ses.stats()
assert st["index16"] and st["index16_fallbacks"] == 0 and st["redone"] == 0, st
g, stride = C.c_void_p(), C.c_int64()
N.check(L.sdfk_dist_gathered(ses.h, C.byref(g), C.byref(stride)))
import torch
raw = np.empty(stride.value, np.uint8)
torch.cuda.synchronize()
import ctypes
hip = ctypes.CDLL("libamdhip64.so")
assert hip.hipMemcpy(ctypes.c_void_p(raw.ctypes.data), g, ctypes.c_size_t(stride.value), 2) == 0
V, Cc, Nn, T, bmin, bmax = D.unpack_self_describing(raw.reshape(1, -1))
assert np.array_equal(T, om.triangles) and np.array_equal(V, om.vertices) and np.array_equal(Nn, om.normals, equal_nan=True)
ses.close()
D.shutdown()
print("index16 fallback ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "index16 fallback ok" in out.stdout, out.stdout[-3000:] + out.stderr[-4000:]


def test_sharded_step_host_cost_world_one(gpu):
    """bench.py's sharded leg on one rank over real RCCL (SDFK_BENCH_FORCE_DIST=1): the line carries the `sharded`
    object with the host microseconds a step costs inside sdfk_dist_submit / sdfk_dist_collect."""
    d = _bench([sys.executable, "bench.py", "--steps", "40", "--warmup", "4", "--no-cpu", "--grid", "128", "--minimal"], {"SDFK_BENCH_FORCE_DIST": "1"})
    sh = d["sharded"]
    assert sh["world"] == 1 and sh["backend"].startswith("RCCL") and sh["steps_redone_on_the_exact_path"] == 0
    # the content check over REAL RCCL (world 1): the mesh the session leaves == sdf.ToMesh of the same grid, SHA-256 of all four arrays
    assert sh["mesh_equals_single_gpu"] is True and sh["content_check"]["every_ranks_slab_equals_its_slice"] is True, sh["content_check"]
    assert sh["every_mesh_equals_single_gpu"] is True
    assert 0 < sh["host_us_per_step"]["submit"] < 200 and sh["host_us_per_step"]["collect"] >= 0
    assert d["config"]["vertices"] > 10000


@pytest.mark.parametrize("world,name,dims,idx16,exchange", [(2, "readme_repeat_xy", (40, 36, 44), 0, 0), (3, "union8", (36, 40, 50), 0, 0), (4, "sphere_w", (64, 64, 64), 0, 0),
                                                            (3, "readme_repeat_xy", (40, 36, 44), 1, 0), (2, "sphere_w", (64, 64, 64), 1, 0),
                                                            (3, "readme_repeat_xy", (40, 36, 44), 0, 3), (2, "union8", (36, 40, 50), 1, 3), (4, "sphere_w", (64, 64, 64), 0, 3),
                                                            (3, "readme_repeat_xy", (40, 36, 44), 0, 2), (2, "union8", (36, 40, 50), 1, 2)])
def test_pipelined_session_full_parity_multi_rank(gpu, world, name, dims, idx16, exchange):
    """2-4 ranks (one GPU, the library's host transport over gloo), real kernels: every rank's whole mesh == the oracle's, bit
    for bit -- with int32 indices rebased by the step, and with the compact 16-bit index payloads decoded by sdfk_dist_mesh.
    exchange 3 = the mesh stays sharded: a step moves the 64-byte headers only; every rank's OWN slab (sdfk_dist_slab_mesh, global
    indices) is its slice of the oracle's mesh, and sdfk_dist_mesh gathers the payloads of that step on demand.
    exchange 2 = gather to rank 0: the other ranks receive headers only, their own sections are never rebased -- their
    sdfk_dist_slab_mesh must still come out with GLOBAL indices (round-5 advisor finding: it did not over RCCL; the host transport
    now has the same who-receives-what as RCCL so that one GPU reaches the path)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join("tests", "multirank_worker.py"), name] + [str(d) for d in dims]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, SDFK_DIST_INDEX16=str(idx16), SDFK_DIST_EXCHANGE=str(exchange)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("identical") == world


def test_bench_contract_fields(gpu):
    """One `--full` bench run (smaller grid, tiny CPU-baseline sample): the JSON line carries
    every field of the contract, the roofline and the cpu_baseline objects."""
    d = _bench([sys.executable, "bench.py", "--full", "--steps", "6", "--warmup", "2", "--grid", "256", "--cpu-n", "64"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["config"]["vertices"] == 137232 and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert abs(d["value"] - 256 ** 3 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 1e-2


def test_default_line_carries_every_baseline_config(gpu):
    """The N = 1 run with `--full` (here without the CPU baseline): beside the 512^3 headline the line carries BASELINE's C2
    (256^3 sphere), C3 (512^3 RepeatXY with colours), C4 (1024^3 union of 8 primitives, whole on one GPU) and C5 (ray marcher), the
    product-default (volume-less) path with a bound of its own, and the controls for the colour sampler."""
    d = _bench([sys.executable, "bench.py", "--full", "--no-cpu", "--steps", "10", "--warmup", "2"], {"SDFK_BENCH_BLOCKS": "3"})
    assert d["config"]["vertices"] == 549144 and d["roofline"]["kernel"] == "sdfk_sample_bits"
    c2, c3, c4 = d["c2_sphere_256"], d["c3_repeatxy"], d["c4_union8_1024"]
    # (the volume-less path needs re-evaluated corners and vertex colours: under SDFK_NO_CORNER_EVAL / SDFK_NO_VCOLOR_EVAL the "product default"
    # legs store the volume like the headline -- tools/gpu_alt_configs.sh runs the suite that way)
    volume_less = not (os.environ.get("SDFK_NO_CORNER_EVAL") or os.environ.get("SDFK_NO_VCOLOR_EVAL"))
    assert c2["vertices"] == 137232 and c2["elided_volume_ms_per_step"] is None and c2["product_default_ms_per_step"] == c2["ms_per_step"]
    assert c3["vertices"] > 900000 and 0 < c3["product_default_ms_per_step"] < c3["ms_per_step"] * (1.0 if volume_less else 1.3)
    assert c4["vertices"] == 3148104 and c4["triangles"] == 6296176 and 0 < c4["product_default_ms_per_step"] < c4["ms_per_step"] * (1.0 if volume_less else 1.3)
    for c in (c2, c3, c4):
        assert c["ms_per_step"] > 0 and 0.2 < c["sampler_frac"] < 1.0 and c["sampler_us_back_to_back"] > 0 and c["mtris_per_s"] > 0
    ctl = d["colour_sampler_control"]
    assert ctl["fill_2gib_us"] > 100 and 0.3 < ctl["fill_2gib_frac_of_peak"] < 1.0 and 0.3 < ctl["trivial_colour_sampler_frac_of_peak"] < 1.0
    assert 0.5 < c3["sampler_frac_of_long_fill"] < 1.5 and 0.5 < c3["sampler_frac_of_trivial_colour_sampler"] < 1.5
    el = d["elided"]
    assert el["ms_per_step"] == d["elided_volume_ms_per_step"] and el["kernels_us"]["k_vertices"]["avg_us"] > 0 and el["chain_serial_us"] > 0
    if volume_less:
        assert "sdfk_cull_blocks" in el["kernels_us"] and "sdfk_eval_blocks" in el["kernels_us"] and "sdfk_sample_bits" not in el["kernels_us"]
    if el["roofline"] is not None:          # (needs the committed SQ counter pass: profiles/pmc_traffic.json)
        assert el["roofline"]["bound"] == "valu" and el["roofline"]["kernel"].startswith("k_vertices") and 0.1 < el["roofline"]["frac"] < 1.0
    assert d["c5_raymarch"]["ms_per_frame"] > 0
    assert 0 < d["one_step_incl_mesh_d2h_product_default_pooled_ms"] <= d["one_step_incl_mesh_d2h_product_default_ms"] * 1.5
    assert d["pipelined_handoff_product_default_ms_per_mesh"] > 0


def _dumped(dirname):
    import numpy as np
    return {name: np.load(os.path.join(dirname, name + ".npy")) for name in ("vertices", "colors", "normals", "triangles", "bounds")}


def test_plain_run_is_the_headline_alone(gpu, tmp_path):
    """Without --full the run sets up, warms up, times its steps, writes --dump-outputs and prints the line: the contract's fields and how
    they were timed, none of the legs beside the headline -- and the mesh it dumps is the mesh a --full run dumps."""
    args = ["--steps", "6", "--warmup", "2", "--grid", "256"]
    d = _bench([sys.executable, "bench.py"] + args + ["--dump-outputs", str(tmp_path / "plain")])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "blocks"):
        assert k in d, k
    assert d["metric"] == "Mvoxels/s, 256^3 sphere SDF sample->mesh" and d["unit"] == "Mvoxels/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["dtype"] == "f32 (sampling) / f64 (cell math)"
    assert d["config"]["vertices"] == 137232
    assert abs(d["value"] - 256 ** 3 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 1e-2
    assert d["blocks"]["ms_per_step_min"] <= d["ms_per_step"] <= d["blocks"]["ms_per_step_max"]
    for k in ("cpu_baseline", "roofline", "kernels_us", "value_cold_clocks", "latency_ms_single_stream", "c2_sphere_256", "c3_repeatxy", "c4_union8_1024",
              "c5_raymarch", "elided", "colour_sampler_control", "hbm_measured", "one_step_incl_mesh_d2h", "host_values_march_ms"):
        assert k not in d, k
    assert "new_constants" not in d["first_call"] and "cold_first_call_ms" not in d["first_call"]
    f = _bench([sys.executable, "bench.py", "--full", "--no-cpu"] + args + ["--dump-outputs", str(tmp_path / "full")])
    assert f["config"] == d["config"] and f["metric"] == d["metric"] and "roofline" in f and "value_cold_clocks" in f
    import numpy as np
    a, b = _dumped(tmp_path / "plain"), _dumped(tmp_path / "full")
    assert a["vertices"].shape == (137232, 3) and all(np.array_equal(a[k], b[k]) for k in a)


def test_plain_sharded_run_on_one_gpu(gpu, tmp_path):
    """`bench.py --gpus 2` without --full (both ranks on this GPU, host transport): the headline of the sharded step and who took part, no
    content check and no pass after the headline; --dump-outputs writes the gathered mesh, which is the single-GPU mesh of the same grid."""
    args = ["--steps", "6", "--warmup", "2", "--grid", "128"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SDFK_BENCH_ONE_GPU"] = "1"
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "2"] + args + ["--dump-outputs", str(tmp_path / "two")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    many = json.loads(lines[0])
    one = _bench([sys.executable, "bench.py"] + args + ["--dump-outputs", str(tmp_path / "one")])
    assert many["n_gpus"] == 2 and many["config"]["vertices"] == one["config"]["vertices"] > 10000
    sh = many["sharded"]
    assert sh["world"] == 2 and sum(p[0] for p in sh["per_rank_vertices_indices"]) == many["config"]["vertices"]
    for k in ("content_check", "mesh_equals_single_gpu", "every_mesh_equals_single_gpu", "c4_union8_1024", "mesh_stays_sharded_pass", "tuned_pass", "slab_kernels_only_ms"):
        assert k not in sh, k
    import numpy as np
    a, b = _dumped(tmp_path / "two"), _dumped(tmp_path / "one")
    assert all(np.array_equal(a[k], b[k]) for k in a)
