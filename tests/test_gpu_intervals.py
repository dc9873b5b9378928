"""The interval arithmetic of the block culling (SDFK_OPT_ELIDE_VOLUME = 2) on the MI355X.

1. Device == host build == model: the text tests/test_interval_codegen.py cuts out of the generated sources, with a probe kernel
   appended (one lane per box writes sdf_interval, one lane per point writes sdf_eval), compiled by hipcc with the optimisation and
   contraction flags lib_jit.hip gives hiprtc, run as ONE child process under a time limit.  Every interval and point value is
   bit-equal to the numpy models, which the CPU file proves bit-equal to the g++ build.  Volume-less programs only: a bound
   program's K.V table and its device-built min/max pyramid cannot be reached without a new entry point; that is out of scope here
   (the device pyramid is covered indirectly by the volume fields of 2).
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
typedef int (*interval_run_fn)(const float* k, int nbox, const float* b, float* iv, int npt, const float* p, float* w);
// one lane per box and one lane per point: whole wavefronts of mixed operands (sdfk_sqrt's ballot takes both paths)
#define INTERVAL_RUN(NK, SETV)                                                                                                 \
    __global__ void probe(const float* k, int nbox, const float* b, float* iv, int npt, const float* p, float* w)              \
    {                                                                                                                          \
        SdfkK K = {};                                                                                                          \
        for (int i = 0; i < NK; i++) K.k[i] = k[i];                                                                            \
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
    static int run(const float* k, int nbox, const float* b, float* iv, int npt, const float* p, float* w)                     \
    {                                                                                                                          \
        const int n = nbox > npt ? nbox : npt;                                                                                 \
        if (n > 0) hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, k, nbox, b, iv, npt, p, w);               \
        return hipDeviceSynchronize() == hipSuccess ? 0 : 1;                                                                   \
    }
"""

PROBE_MAIN = r"""
static FILE* g_in;
template <class T> static std::vector<T> rd(size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, g_in) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
template <class T> static T* up(const std::vector<T>& v, size_t atleast)
{
    T* d = nullptr;
    const size_t n = v.size() > atleast ? v.size() : atleast;
    if (hipMalloc(&d, (n ? n : 1) * sizeof(T)) != hipSuccess) { fprintf(stderr, "hipMalloc\n"); exit(3); }
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
        if (h[0] < 0 || h[0] >= nprog || h[2] != 0) { fprintf(stderr, "bad record\n"); return 2; }
        std::vector<float> k = rd<float>((size_t)h[1]), b = rd<float>(6 * (size_t)h[3]), p = rd<float>(3 * (size_t)h[4]);
        std::vector<float> iv(2 * (size_t)h[3]), w((size_t)h[4]);
        float *dk = up(k, 1), *db = up(b, 0), *dp = up(p, 0), *div = up(iv, 0), *dw = up(w, 0);
        if (kPrograms[h[0]](dk, h[3], db, div, h[4], dp, dw)) { fprintf(stderr, "kernel failed, program %d\n", h[0]); return 3; }
        if (iv.size() && hipMemcpy(iv.data(), div, iv.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
        if (w.size() && hipMemcpy(w.data(), dw, w.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
        hipFree(dk); hipFree(db); hipFree(dp); hipFree(div); hipFree(dw);
        fwrite(iv.data(), 4, iv.size(), out);
        fwrite(w.data(), 4, w.size(), out);
        n++;
    }
    fclose(out);
    printf("interval ok %d\n", n);
    return 0;
}
"""


def test_device_equals_host_build_equals_model(gpu, codegen, tmp_path):
    """Every volume-less program of the CPU file (catalogue, mathops scenes, the random DAGs, the domain-safe DAGs, one program per
    opcode), on the same boxes and points: the device's sdf_interval and sdf_eval are bit-equal to the models.  Bound programs are
    out of scope (see the module docstring)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "no hipcc"
    programs = [p for p in T.whole_programs() + T.single_op_programs() if not p["vols"]]
    t = T.Text(codegen, programs)
    assert not t.vol
    src = tmp_path / "probe.hip"
    src.write_text(PROBE_HEAD + t.unit() + PROBE_MAIN)
    exe = tmp_path / "probe"
    # -O3 -ffp-contract=off -DSDFK_SAMPLE_NT=1 -DSDFK_SAMPLE_RPW=kSampleRpw (lib_internal.h: 2): the options lib_jit.hip gives hiprtc
    c = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-DSDFK_KERNELS=0x200", "-DSDFK_SAMPLE_NT=1",
                        "-DSDFK_SAMPLE_RPW=2", "-std=c++17", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-4000:]
    tables = T.edge_tables()
    recs, meta = [], []
    for n, p in enumerate(programs):
        if p["name"] in tables:
            B = tables[p["name"]]
            pts = T.edge_points(p["name"], B[:4096]).reshape(-1, 3)
        else:
            B, nsub, ncoarse = T.program_boxes(p)
            pts = np.concatenate(T.program_points(p, B, nsub, ncoarse))
        recs.append((n, t.cuts[n][3], [], B, pts))
        meta.append((B, pts))
    fin, fout = str(tmp_path / "in"), str(tmp_path / "out")
    T.write_records(fin, recs)
    r = subprocess.run(["timeout", "-k", "10", "300", str(exe), fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and "interval ok" in r.stdout, (r.returncode, r.stdout, r.stderr)   # (nothing else touches the GPU after a failure here)
    for p, (B, pts), (iv, w) in zip(programs, meta, T.read_results(fout, recs)):
        lo, hi = T.model_interval(p, B)
        bad = ~(T.bits_eq(iv[:, 0], lo) & T.bits_eq(iv[:, 1], hi))
        assert not bad.any(), (p["name"], "device interval != model", B[bad][:3], iv[bad][:3], lo[bad][:3], hi[bad][:3])
        want = T.point_values(p, pts)
        bad = ~T.bits_eq(w, want)
        assert not bad.any(), (p["name"], "device sdf_eval != model", pts[bad][:3], w[bad][:3], want[bad][:3])


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
