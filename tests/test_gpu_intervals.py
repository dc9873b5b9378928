"""The interval arithmetic of the block culling (SDFK_OPT_ELIDE_VOLUME = 2) on the MI355X.

1. Device == host build == model: the text tests/test_interval_codegen.py cuts out of the generated sources, with a probe kernel
   appended (one lane per box writes sdf_interval, one lane per point writes sdf_eval), compiled by hipcc with the optimisation and
   contraction flags lib_jit.hip gives hiprtc, run as ONE child process under a time limit.  Every interval and point value is
   bit-equal to the numpy models, which the CPU file proves bit-equal to the g++ build.  Bound programs included: the probe
   uploads each volume of a record (pitched values and colours), builds the min/max pyramid of every channel ON THE DEVICE with
   csrc/vol_pyramid.h -- the kernels and the launcher bind_volumes uses -- and points an SdfkVol table at it; the record's model
   pyramid is read past.  The built pyramids come back and are bit-equal, level by level and NaN cell by NaN cell, to
   voxel_sdf_model.pyramid; iv_vox_nearest / iv_vox_linear / iv_vox_box then read the device's pyramid, not the model's.
   The volumes are those of the CPU file: the bound scenes, the edge volumes, and the shapes at which a level can go wrong (no
   pyramid at all, a clipped last cell at every level, N = 1 and N = 2 axes, non-finite corner voxels with padded rows, one NaN
   in a power of two, and 176 x 160 x 160, whose level 1 needs the second step of the base kernel's grid stride).
   What this catches, established by reverting vol_pyramid.h locally and running once: see test_device_equals_host_build_equals_model.
   What it does not reach -- bind_volumes' own layout (one pyramid per channel read, one block per slot) -- is
   tests/test_gpu_voxel_cull.py's.
2. Meshes that a one-ulp error changes: one-line fields on a 264 x 260 x 256 grid, isoValue set to the float just below the largest
   voxel of an interior 8 x 4 x 4 sub-box (only its extreme voxels lie above), and to the smallest voxel itself (`<= iso` is the
   tie): culled (mode 2) == sign-only (mode 1) == stored (mode 0), bit for bit, and different from the mesh at the neighbouring iso.
   What these cases can and cannot catch, established by reverting the product locally (see _check_one_ulp_cases).
3. Culling still culls: the work-list counter is not exposed by the ABI; what is observable (sdfk_cull_blocks and sdfk_eval_blocks
   ran) is asserted here, and the share of sub-boxes the MODEL decides per scene is the CPU-side number asserted in
   tests/test_interval_codegen.py::test_culler_boxes_contain_the_sampled_volume."""
import os
import subprocess

import numpy as np
import pytest

from sdfkit_amd import _native as N
from sdfkit_amd import Voxels
from sdfkit_amd.api import Sdf
from sdfkit_amd.expr import MathF, Mod, Vec4, select_lt
from tests import mathops_model as M
from tests import scenes as S
from tests import test_interval_codegen as T
from tests import voxel_sdf_model as VM
from tests.test_gpu_elide_volume import _kernels_launched, _same_mesh
from tests.test_voxel_sdf_codegen import codegen  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32

PROBE_HEAD = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "vol_pyramid.h"
typedef int (*interval_run_fn)(const float* k, const void* V, int nbox, const float* b, float* iv, int npt, const float* p, float* w);
// one lane per box and one lane per point: whole wavefronts of mixed operands (sdfk_sqrt's ballot takes both paths)
#define INTERVAL_RUN(NK, SETV)                                                                                                 \
    __global__ void probe(const float* k, const void* V, int nbox, const float* b, float* iv, int npt, const float* p, float* w) \
    {                                                                                                                          \
        SdfkK K = {};                                                                                                          \
        for (int i = 0; i < NK; i++) K.k[i] = k[i];                                                                            \
        (void)V;                                                                                                               \
        SETV                                                                                                                   \
        const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;                                                            \
        if (i < nbox) {                                                                                                        \
            sdfk_iv X, Y, Z;                                                                                                   \
            X.lo = b[6 * i]; X.hi = b[6 * i + 1]; Y.lo = b[6 * i + 2]; Y.hi = b[6 * i + 3]; Z.lo = b[6 * i + 4]; Z.hi = b[6 * i + 5]; \
            const sdfk_iv r = sdf_interval(K, X, Y, Z);                                                                        \
            iv[2 * i] = r.lo; iv[2 * i + 1] = r.hi;                                                                            \
        }                                                                                                                      \
        if (i < npt) {                                                                                                         \
            float R, G, B, W;                                                                                                  \
            sdf_eval(K, p[3 * i], p[3 * i + 1], p[3 * i + 2], R, G, B, W);                                                     \
            w[i] = W;                                                                                                          \
        }                                                                                                                      \
    }                                                                                                                          \
    static int run(const float* k, const void* V, int nbox, const float* b, float* iv, int npt, const float* p, float* w)      \
    {                                                                                                                          \
        const int n = nbox > npt ? nbox : npt;                                                                                 \
        if (n > 0) hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, k, V, nbox, b, iv, npt, p, w);            \
        return hipDeviceSynchronize() == hipSuccess ? 0 : 1;                                                                   \
    }
"""

# IN: the records of tests/cpp/interval_host.cpp.  OUT, per record: per volume, per channel 0..3 (3 only without colours), the
# pyramid the device built (levels 1..nlev, (lo, hi) per cell); then float iv[nbox][2], float w[npt].
PROBE_MAIN = r"""
static FILE* g_in;
template <class T> static std::vector<T> rd(size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, g_in) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
static std::vector<void*> g_dev;   // the device arrays of one record
template <class T> static T* dev(size_t n)
{
    T* d = nullptr;
    if (hipMalloc(&d, (n ? n : 1) * sizeof(T)) != hipSuccess) { fprintf(stderr, "hipMalloc\n"); exit(3); }
    g_dev.push_back(d);
    return d;
}
template <class T> static T* up(const std::vector<T>& v)
{
    T* d = dev<T>(v.size());
    if (v.size() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "hipMemcpy\n"); exit(3); }
    return d;
}
int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    g_in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!g_in || !out) return 2;
    const int nprog = (int)(sizeof kPrograms / sizeof kPrograms[0]);
    int n = 0;
    for (;;) {
        int32_t h[5];
        if (fread(h, sizeof h, 1, g_in) != 1) break;
        if (h[0] < 0 || h[0] >= nprog || h[2] < 0 || h[2] > 8) { fprintf(stderr, "bad record\n"); return 2; }
        std::vector<float> k = rd<float>((size_t)h[1]);
        const void* table = nullptr;
#ifdef INTERVAL_HAS_VOLUMES
        std::vector<SdfkVol> vols((size_t)h[2]);
        for (SdfkVol& V : vols) {
            memset(&V, 0, sizeof V);
            std::vector<int32_t> q = rd<int32_t>(6);
            std::vector<float> g = rd<float>(9);
            if (q[0] < 1 || q[1] < 1 || q[2] < 1 || q[3] < q[2]) { fprintf(stderr, "bad volume\n"); return 2; }
            for (int a = 0; a < 3; a++) { V.n[a] = q[a]; V.mn[a] = g[a]; V.d[a] = g[3 + a]; V.m[a] = g[6 + a]; }
            V.pitch = q[3];
            const size_t nalloc = (size_t)q[0] * q[1] * q[3];
            float* val = up(rd<float>(nalloc));
            float* col = q[4] ? up(rd<float>(3 * nalloc)) : nullptr;
            V.val = val;
            V.col = col;
            const long long total = vol_pyr_levels(V.n, &V.nlev, V.lev);
            if (V.nlev != q[5]) { fprintf(stderr, "nlev %d, the record has %d\n", V.nlev, q[5]); return 2; }
            for (int ch = q[4] ? 0 : 3; ch < 4; ch++) {
                for (int L = 1; L <= q[5]; L++) rd<float>(2 * (size_t)rd<int32_t>(1)[0]);   // (the model's pyramid: read past)
                if (V.nlev == 0) continue;
                std::vector<float> P(2 * (size_t)total);
                float* dP = dev<float>(P.size());
                if (hipMemset(dP, 0x55, P.size() * 4) != hipSuccess) return 3;   // (a cell nobody writes stays 1.46e13)
                const float* src = ch == 3 ? val : col + ch;
                if (vol_pyr_build(src, ch == 3 ? 1 : 3, V.n, V.pitch, V.nlev, V.lev, dP, 0) != hipSuccess) { fprintf(stderr, "vol_pyr_build\n"); return 3; }
                if (hipMemcpy(P.data(), dP, P.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "pyramid kernels failed\n"); return 3; }
                fwrite(P.data(), 4, P.size(), out);
                V.pyr[ch] = dP;
            }
        }
        table = up(vols);
#else
        if (h[2]) { fprintf(stderr, "built without volumes\n"); return 2; }
#endif
        std::vector<float> b = rd<float>(6 * (size_t)h[3]), p = rd<float>(3 * (size_t)h[4]);
        std::vector<float> iv(2 * (size_t)h[3]), w((size_t)h[4]);
        float *dk = up(k), *db = up(b), *dp = up(p), *div = up(iv), *dw = up(w);
        if (kPrograms[h[0]](dk, table, h[3], db, div, h[4], dp, dw)) { fprintf(stderr, "kernel failed, program %d\n", h[0]); return 3; }
        if (iv.size() && hipMemcpy(iv.data(), div, iv.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
        if (w.size() && hipMemcpy(w.data(), dw, w.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
        for (void* d : g_dev) (void)hipFree(d);
        g_dev.clear();
        fwrite(iv.data(), 4, iv.size(), out);
        fwrite(w.data(), 4, w.size(), out);
        n++;
    }
    fclose(out);
    printf("interval ok %d\n", n);
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(codegen, tmp_path_factory):
    """(Text, executable) of every program of the CPU file -- catalogue, mathops scenes, the random DAGs, the domain-safe DAGs, the
    bound scenes, one program per opcode and per edge volume -- built once"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "no hipcc"
    t = T.Text(codegen, T.whole_programs() + T.single_op_programs())
    assert t.vol
    d = tmp_path_factory.mktemp("interval_probe")
    src, exe = d / "probe.hip", d / "probe"
    src.write_text(PROBE_HEAD + t.unit() + PROBE_MAIN)
    # -O3 -ffp-contract=off -DSDFK_SAMPLE_NT=1 -DSDFK_SAMPLE_RPW=kSampleRpw (lib_internal.h: 2): the options lib_jit.hip gives hiprtc
    c = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-DSDFK_KERNELS=0x200", "-DSDFK_SAMPLE_NT=1",
                        "-DSDFK_SAMPLE_RPW=2", "-DINTERVAL_HAS_VOLUMES", "-std=c++17", "-I", os.path.join(T.ROOT, "sdfkit_amd", "csrc"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-4000:]
    return t, str(exe)


def _channels(vol):
    return range(4) if vol[1] is not None else (3,)


def _run_probe(exe, d, tag, recs, padding="nan"):
    """one child process: [(pyramids {(volume, channel): flat floats}, iv [nbox, 2], w [npt])] per record"""
    fin, fout = str(d / f"in_{tag}"), str(d / f"out_{tag}")
    T.write_records(fin, recs, padding=padding)
    r = subprocess.run(["timeout", "-k", "10", "300", exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and "interval ok" in r.stdout, (r.returncode, r.stdout, r.stderr)   # (nothing else touches the GPU after a failure here)
    data, o, res = np.fromfile(fout, f32), 0, []
    for _, _, vols, boxes, pts in recs:
        pyr = {}
        for vi, vol in enumerate(vols):
            cells = sum(lo.size for lo, _ in VM.pyramid(vol[0])[1:])
            for ch in (_channels(vol) if cells else ()):
                pyr[(vi, ch)] = data[o:o + 2 * cells]
                o += 2 * cells
        nb, npt = len(boxes), len(pts)
        res.append((pyr, data[o:o + 2 * nb].reshape(nb, 2), data[o + 2 * nb:o + 2 * nb + npt]))
        o += 2 * nb + npt
    assert o == len(data)
    return res


_MODEL_PYRAMIDS = {}


def _model_pyramid(vol, ch):
    """voxel_sdf_model.pyramid of a channel, computed once per volume: [(lo, hi)] for the levels 1..top"""
    key = (id(vol), ch)
    if key not in _MODEL_PYRAMIDS:
        _MODEL_PYRAMIDS[key] = (vol, VM.pyramid(VM._channel(vol, ch))[1:])
    return _MODEL_PYRAMIDS[key][1]


def _assert_pyramids(name, vols, pyr):
    """every level of every channel the device built, on bits (NaN == NaN): a poisoned cell must be poisoned, and no other"""
    for vi, vol in enumerate(vols):
        levels = _model_pyramid(vol, 3)
        assert sorted(c for v, c in pyr if v == vi) == (list(_channels(vol)) if levels else []), (name, vi)
        for ch in (_channels(vol) if levels else ()):
            o = 0
            for L, (lo, hi) in enumerate(_model_pyramid(vol, ch), 1):
                got = pyr[(vi, ch)][o:o + 2 * lo.size].reshape(lo.shape + (2,))
                o += 2 * lo.size
                assert np.array_equal(np.isnan(got[..., 0]), np.isnan(lo)) and np.array_equal(np.isnan(got[..., 1]), np.isnan(hi)), \
                    (name, vol[0].shape, ch, L, "the poisoned cells differ", np.argwhere(np.isnan(got[..., 0]) != np.isnan(lo))[:4])
                bad = ~(T.bits_eq(got[..., 0], lo) & T.bits_eq(got[..., 1], hi))
                assert not bad.any(), (name, vol[0].shape, ch, L, "device pyramid != model", np.argwhere(bad)[:4], got[bad][:4], lo[bad][:4], hi[bad][:4])
            assert o == len(pyr[(vi, ch)])


def _assert_values(p, B, pts, iv, w):
    lo, hi = T.model_interval(p, B)
    bad = ~(T.bits_eq(iv[:, 0], lo) & T.bits_eq(iv[:, 1], hi))
    assert not bad.any(), (p["name"], "device interval != model", B[bad][:3], iv[bad][:3], lo[bad][:3], hi[bad][:3])
    want = T.point_values(p, pts)
    bad = ~T.bits_eq(w, want)
    assert not bad.any(), (p["name"], "device sdf_eval != model", pts[bad][:3], w[bad][:3], want[bad][:3])


def _records(t, select=lambda p: True):
    tables = T.edge_tables()
    recs, meta = [], []
    for n, p in enumerate(t.programs):
        if not select(p):
            continue
        if p["name"] in tables:
            B = tables[p["name"]]
            pts = T.edge_points(p["name"], B[:4096]).reshape(-1, 3)
        else:
            B, nsub, ncoarse = T.program_boxes(p)
            pts = np.concatenate(T.program_points(p, B, nsub, ncoarse))
        recs.append((n, t.cuts[n][3], p["vols"], B, pts))
        meta.append((p, B, pts))
    return recs, meta


def test_device_equals_host_build_equals_model(gpu, probe, tmp_path):
    """Every program of the CPU file (catalogue, mathops scenes, the random DAGs, the domain-safe DAGs, the bound scenes, one program
    per opcode and per edge volume), on the same boxes and points: the device's sdf_interval and sdf_eval are bit-equal to the
    models, and so is every level of every pyramid the device built for a bound program's volumes.

    What this catches, found by making each change in csrc/vol_pyramid.h (none reads outside an allocation), building and running
    this test and test_row_padding_is_never_read once; both failed every time, on a pyramid comparison:
      k_vol_pyr_up skips child q == 7              device pyramid != model at level 2 (bound_two_volumes' 12 x 10 x 14, first)
      __builtin_elementwise_minimum -> fminf       the poisoned cells differ at level 2 (65 x 33 x 17, colour channel 1): lo loses
                                                   the NaN, hi keeps it.  No mesh can show this one: iv_whole makes the interval
                                                   unknown from hi alone, so tests/test_gpu_voxel_cull.py passes with it
      k_vol_pyr_base without the `bad` poison      the poisoned cells differ at level 1 (the +-inf voxels of 13 x 6 x 21 and
                                                   65 x 33 x 17; a NaN voxel poisons through minimum / maximum anyway).  No mesh of
                                                   tests/test_gpu_voxel_cull.py shows it either: a read's result is clamped to its
                                                   corners, so [c, inf] still contains it
      lev[] starts one level late                  the probe's output no longer has the layout's size
    (the fifth, channel 1's pyramid built from channel 0, is a change of bind_volumes: tests/test_gpu_voxel_cull.py)"""
    t, exe = probe
    assert sum(bool(p["vols"]) for p in t.programs) >= 3 + 2 * len(T.EDGE_VOLS)
    recs, meta = _records(t)
    for (p, B, pts), (pyr, iv, w) in zip(meta, _run_probe(exe, tmp_path, "all", recs)):
        _assert_pyramids(p["name"], p["vols"], pyr)
        _assert_values(p, B, pts, iv, w)


def test_row_padding_is_never_read(gpu, probe, tmp_path):
    """65 x 33 x 17 (rows of 17 in a pitch of 20), its values and colour channel 1 through both reads, run twice: the padding NaN, and
    alternately +FLT_MAX and -FLT_MAX.  Both runs give the model's pyramid, intervals and point values, hence the same: a read into
    the padding cannot hide behind a NaN that a minimum or a select then drops."""
    t, exe = probe
    vol = T.EDGE_VOLS[T.POISONED_VOL]
    recs, meta = _records(t, lambda p: len(p["vols"]) == 1 and p["vols"][0] is vol)
    assert len(recs) == 4 and T.volume_record(vol, "nan") != T.volume_record(vol, "fmax")
    runs = {}
    for padding in ("nan", "fmax"):   # (one child each; the second is not started when the first fails)
        runs[padding] = _run_probe(exe, tmp_path, padding, recs, padding)
        for (p, B, pts), (pyr, iv, w) in zip(meta, runs[padding]):
            _assert_pyramids(p["name"] + " padding " + padding, p["vols"], pyr)
            _assert_values(p, B, pts, iv, w)
    for (pa, iva, wa), (pb, ivb, wb) in zip(runs["nan"], runs["fmax"]):
        assert all(np.all(T.bits_eq(pa[k], pb[k])) for k in pa) and np.all(T.bits_eq(iva, ivb)) and np.all(T.bits_eq(wa, wb))


# ---- meshes that a one-ulp error changes ----------------------------------------------------------------------------------------
BOX = ([-1.5, -1.5, -1.5], [1.5, 1.5, 1.5])
DIMS = (264, 260, 256)


def _flat(w, p):
    """a field of x (and z) alone still has to be a value of all three coordinates for the tracer: + 0 y"""
    return Vec4.of((1.0, 1.0, 1.0), w + p.y * 0.0)


FIELDS = {
    # maxima of sin(s x) between, on and next to sample points: s chosen so that s x walks through many residues
    "sin": lambda p: _flat(MathF.Sin(p.x * 7.3), p),
    "sin_3d": lambda p: Vec4.of((1.0, 1.0, 1.0), MathF.Sin(p.x * 5.0) * MathF.Cos(p.y * 3.0) + p.z * 0.0),
    # arguments on both sides of 2^22 (the two reductions of sdfk_m_reduce), a quarter to half a radian apart: a staircase of x
    "cos_4e6": lambda p: _flat(MathF.Cos(p.x * 2.0 + 4194304.0), p),
    "exp": lambda p: Vec4.of((1.0, 1.0, 1.0), MathF.Exp(p.Length() * -2.0)),
    "log": lambda p: _flat(MathF.Log(abs(p.x) + 0.25), p),
    "atan2": lambda p: _flat(MathF.Atan2(p.z, p.x), p),
    "sqrt": lambda p: Vec4.of((1.0, 1.0, 1.0), p.Length() - 1.0),
    "div": lambda p: Vec4.of((1.0, 1.0, 1.0), 1.0 / (p.Length() + 0.5)),
    "mod": lambda p: _flat(Mod(p.x, 0.7) + p.z * 0.125, p),
    "sel_lt": lambda p: Vec4.of((1.0, 1.0, 1.0), select_lt(p.x, p.y, p.Length() - 1.0, p.z * 0.5)),
}


def _sub_boxes(W):
    """interior 8 x 4 x 4 sub-boxes of whole blocks, away from the clipped faces: the one holding the field's largest interior value,
    the one holding its smallest, and two fixed ones"""
    nx, ny, nz = W.shape
    inner = W[64:(nx // 64 - 1) * 64, 8:ny - 8, 8:nz - 8]
    fin = np.where(np.isfinite(inner), inner, np.nan)
    picks = []
    for at in (np.nanargmax(fin), np.nanargmin(fin)):
        i, j, k = np.unravel_index(at, inner.shape)
        picks.append(((i + 64) // 8, (j + 8) // 4, (k + 8) // 4))
    return picks + [(11, 23, 17), (20, 40, 45)]


def _check_one_ulp_cases(sdf, W, name):
    """A decision of the culling pass that is wrong by one ulp, by a missed extremum or by a wrong `<=` changes these meshes: that
    holds for the operations whose interval ends are exact (sqrt, div, floor, sel_lt, the volume reads) and for the extremum and
    cut logic of sin / cos / atan2.  It does NOT hold for the one-ulp widening of the faithful functions (sdfk_succ / sdfk_pred in
    iv_sincos, iv_exp, iv_log, iv_atan2): the ends of the culler's boxes ARE sample points, so without the widening hi is still
    the largest voxel itself, which is above an iso one ulp below it, and lo is the smallest voxel, which is not above an iso
    equal to it; the box stays undecided either way.  Only an interior voxel exceeding both ends' values (f^ non-monotone by an
    ulp) could show, and these fields have none.  Reverting `sdfk_succ(fh)` in iv_sincos and `sdfk_pred(sdfk_logf(a.lo))` in iv_log
    in the product leaves every case here passing; tests/test_interval_codegen.py catches both (text != model).  The 0 * inf line
    of iv_mul needs an infinity: test_mesh_with_zero_times_infinity below."""
    n_cases = 0
    for (s, t, u) in _sub_boxes(W):
        v = W[8 * s:8 * s + 8, 4 * t:4 * t + 4, 4 * u:4 * u + 4]
        if not np.all(np.isfinite(v)) or v.max() == v.min():
            continue
        # just below the largest voxel (only the extreme voxels lie above); the smallest itself (`<= iso` is the tie)
        for iso, other in ((M.pred(f32(v.max())), f32(v.max())), (f32(v.min()), M.pred(f32(v.min())))):
            meshes = {}
            for mode in (0, 1, 2):
                with N.option(N.OPT_ELIDE_VOLUME, mode):
                    if mode == 2:
                        meshes[mode], ran = _kernels_launched(lambda: sdf.ToMesh(*BOX, *DIMS, isoValue=float(iso)))
                        assert "sdfk_cull_blocks" in ran and "sdfk_eval_blocks" in ran, ran
                    else:
                        meshes[mode] = sdf.ToMesh(*BOX, *DIMS, isoValue=float(iso))
            assert _same_mesh(meshes[2], meshes[0]), (name, (s, t, u), float(iso), "culled != stored")
            assert _same_mesh(meshes[1], meshes[0]), (name, (s, t, u), float(iso), "sign-only != stored")
            with N.option(N.OPT_ELIDE_VOLUME, 0):
                nb = sdf.ToMesh(*BOX, *DIMS, isoValue=float(other))
            assert not _same_mesh(nb, meshes[0]), (name, (s, t, u), float(iso), "the extreme voxels produce no geometry")
            n_cases += 1
    assert n_cases >= 4, (name, n_cases)


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_meshes_that_a_one_ulp_error_changes(gpu, name):
    sdf = Sdf(FIELDS[name], True)
    W = sdf.ToVoxels(*BOX, *DIMS, clipToBounds=False).Values   # (the stored volume: its parity with the model is test_gpu_mathops')
    _check_one_ulp_cases(sdf, W, name)


@pytest.mark.parametrize("interpolate", [False, True])
def test_volume_read_meshes_that_a_one_ulp_error_changes(gpu, interpolate):
    """a smooth volume (a sphere's distance, 40 x 36 x 44) read through both index maps: the device-built pyramid decides the boxes"""
    vals, _, mn, mx = T._sphere_volume((40, 36, 44), (-1.25,) * 3, (1.25,) * 3, False, 0)
    sdf = Voxels(vals, None, mn, mx).ToSdf(interpolate)
    W = sdf.ToVoxels(*BOX, *DIMS, clipToBounds=False).Values
    _check_one_ulp_cases(sdf, W, f"voxels_{interpolate}")


def test_mesh_with_zero_times_infinity(gpu):
    """max(x * inf, 1): 1 for x < 0, inf for x > 0, NaN on the plane of sample points x == 0 (the grid is placed so that sample 100
    of x is exactly 0).  A sub-box through x = 0 has corner products -inf and +inf only; without iv_mul's `0 * inf somewhere in the
    box` line its interval is [1, inf], the box is decided "above 0" and the NaN voxels (not above) lose their geometry.  Caught
    when that line is reverted in the product: culled != stored here."""
    inf = float("inf")
    sdf = Sdf(lambda p: Vec4.of((1.0, 1.0, 1.0), MathF.Max(p.x * inf, 1.0) + (p.y + p.z) * 0.0), True)
    x0 = -100.5 / 128
    mn, mx = [x0, -1.5, -1.5], [x0 + 264 / 128, 1.5, 1.5]
    W = sdf.ToVoxels(mn, mx, *DIMS, clipToBounds=False).Values
    assert np.isnan(W[100]).all() and np.all(W[:100] == 1) and np.all(W[101:] == np.inf)
    meshes = {}
    for mode in (0, 1, 2):
        with N.option(N.OPT_ELIDE_VOLUME, mode):
            meshes[mode] = sdf.ToMesh(mn, mx, *DIMS, isoValue=0.0)
    assert len(meshes[0].Triangles) > 1000
    assert _same_mesh(meshes[2], meshes[0]), "culled != stored"
    assert _same_mesh(meshes[1], meshes[0]), "sign-only != stored"


# ---- culling still culls --------------------------------------------------------------------------------------------------------
def _cull_scenes():
    from tests.test_gpu_mathops import BOX as MBOX, SCENES
    res = {k: (lambda k=k: S.CATALOGUE[k]()[1], ([-2.8125] * 3, [2.8125] * 3)) for k in S.CATALOGUE}
    res.update({k: (lambda fn=fn: Sdf(fn, True), MBOX) for k, fn in SCENES.items()})
    return res


@pytest.mark.parametrize("name", sorted(_cull_scenes()))
def test_culling_pass_runs(gpu, name):
    """the observable half of "culling still culls" for the twelve catalogue scenes and the four mathops scenes (the work-list
    counter is not exposed): with the product default both culling kernels run and no dense sampler does; the decided share is the
    model's, asserted on the CPU"""
    mk, box = _cull_scenes()[name]
    sdf = mk()
    _, ran = _kernels_launched(lambda: sdf.ToMesh(*box, *DIMS))
    assert "sdfk_cull_blocks" in ran and "sdfk_eval_blocks" in ran and not any(k.startswith("sdfk_sample_") for k in ran), ran
