"""CPU check of the redistancing arithmetic (sdfkit_amd/csrc/redistance.h, the functions the kernels of lib_redistance.hip call,
built with g++ -O2 -ffp-contract=off as a full-sweep Jacobi solver by tests/cpp/redistance_host.cpp) against the numpy model
(tests/redistance_model.py), bit for bit: the spheres, seeded random volumes (fronts everywhere), random anisotropic boxes,
bands and iso values."""
import numpy as np
import pytest

from tests import redistance_model as M

f32 = np.float32


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return M.build_host_solver(tmp_path_factory.mktemp("redistance"))


def _same(exe, tmp_path, v, h, iso=0.0, band=np.inf):
    got, gst = M.host_solve(exe, v, h, iso, band, tmp_path)
    want, wst = M.redistance(v, h, iso, band)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[:4].T)], want[tuple(bad[:4].T)])
    assert gst == {k: wst[k] for k in gst}
    return wst


@pytest.mark.parametrize("n", [16, 32, 64])
def test_spheres_match_model_bitwise(host_exe, tmp_path, n):
    for kind in ("abc" if n < 64 else "c"):
        v, h, _ = M.sphere_inputs(n, kind)
        _same(host_exe, tmp_path, v, h)


@pytest.mark.parametrize("seed", range(8))
def test_random_volumes_match_model_bitwise(host_exe, tmp_path, seed):
    v = np.random.default_rng(seed).uniform(-1, 1, (17, 17, 17)).astype(f32)
    st = _same(host_exe, tmp_path, v, np.ones(3, f32))
    assert st["front"] > v.size // 2


@pytest.mark.parametrize("seed", range(6))
def test_random_anisotropic_boxes_match_model_bitwise(host_exe, tmp_path, seed):
    rng = np.random.default_rng(100 + seed)
    shape = tuple(int(x) for x in rng.integers(5, 30, 3))
    h = rng.uniform(0.01, 2.0, 3).astype(f32)
    x, y, z = np.meshgrid(*[np.arange(n) * float(d) for n, d in zip(shape, h)], indexing="ij")
    c = [rng.uniform(0, n * float(d)) for n, d in zip(shape, h)]
    v = (rng.uniform(0.5, 4.0) * (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - 0.3 * max(c)) +
         rng.uniform(-0.1, 0.1, shape) * float(h.min())).astype(f32)
    iso = float(rng.uniform(-0.1, 0.1))
    full = _same(host_exe, tmp_path, v, h, iso)
    _same(host_exe, tmp_path, v, h, iso, band=float(f32(2.5) * h.max()))
    assert full["sweeps"] >= 1


def test_degenerate_inputs_match_model_bitwise(host_exe, tmp_path):
    v = np.ones((6, 5, 4), f32)
    _same(host_exe, tmp_path, v, np.ones(3, f32))                      # no front
    _same(host_exe, tmp_path, -v, np.ones(3, f32), band=0.5)
    v[2:4, 1:3, 1:3] = 0.0                                             # == iso: T0 = 0, -0.0
    _same(host_exe, tmp_path, v, np.array([0.5, 1.0, 2.0], f32))
    _same(host_exe, tmp_path, v, np.array([0.5, 1.0, 2.0], f32), band=0.0)
    tiny = np.array([1e-30, -1e-38, 3e38, -3e38], f32).reshape(4, 1, 1) * np.ones((4, 3, 2), f32)   # extreme magnitudes
    _same(host_exe, tmp_path, tiny, np.array([1e-3, 1.0, 1e3], f32))
