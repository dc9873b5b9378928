"""SDFK_OPT_COUNT_BYTES: a sdfk_sample_march job (SdfEx.ToMesh) whose sampler has just written the sign bytes of its own volume counts
its active cells straight from those bytes (k_count_bytes: lanes along z, the 8 x 8 byte transposition in registers) instead of
regrouping them into words first (k_bits_transpose) and counting from the words (k_compact).  The old kernels are the
reference here: with the option off the very same call takes them, and the four mesh arrays, the bounds and both cell counts must
come out byte for byte the same.  Shapes: one lane (nz = 8), the hand-over between lanes (16), a full 512-layer chunk and the chunk
boundary (520), one, two and three words per row with a partial last word (nx = 64, 72, 130), enough segments for a second quarter
and a second block part, ClipToBounds on and off, case-13 sign words, the README scene.  That a shape the kernel does not cover (a byte
pitch that is no multiple of 8) keeps the old kernels, and that the counts a job ADDS into are zero again for the next job on the same
stream, is checked as well."""
import numpy as np
import pytest

from sdfkit_amd import Sdfs
from sdfkit_amd import _native as N
from sdfkit_amd.api import Sdf
from sdfkit_amd.expr import MathF, Vec4
from tests import scenes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    N.init(0)
    return True


def _kernels_launched(fn):
    L = N.lib()
    N.check(L.sdfk_profile_reset())
    N.check(L.sdfk_profile_enable(1))     # (a profiled job is never a captured graph: the ordinary path, whatever the grid size)
    try:
        out = fn()
    finally:
        N.check(L.sdfk_profile_enable(0))
    return out, {k for k, v in N.profile_snapshot().items() if v[1]}


def _assert_same(a, b, what):
    bits = lambda x: np.ascontiguousarray(x).view(np.uint8)
    for name in ("Vertices", "Colors", "Normals", "Triangles", "Min", "Max"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), (what, name, x.shape, y.shape)
    assert a.ActiveCells == b.ActiveCells and a.ImpossibleCase13Cells == b.ImpossibleCase13Cells, (what, a.ActiveCells, b.ActiveCells)


def _both_paths(sdf, mn, mx, dims, clip, expect_new=True, elide=0, reps=2):
    """the forced old path, then the new one `reps` times (exact two-phase job first, then the speculative one)"""
    with N.option(N.OPT_ELIDE_VOLUME, elide):
        with N.option(N.OPT_COUNT_BYTES, 0):
            ref, ran = _kernels_launched(lambda: sdf.ToMesh(mn, mx, *dims, clipToBounds=clip))
            assert "k_bits_transpose" in ran and "k_compact" in ran, ran
        with N.option(N.OPT_COUNT_BYTES, 1):
            for rep in range(reps):
                got, ran = _kernels_launched(lambda: sdf.ToMesh(mn, mx, *dims, clipToBounds=clip))
                assert ("k_bits_transpose" not in ran) == expect_new and "k_compact" in ran, (dims, rep, ran)
                _assert_same(got, ref, (dims, clip, rep))
    return ref


SHAPES = [(16, 16, 8), (16, 16, 16), (16, 16, 512), (16, 16, 520), (64, 16, 16), (72, 16, 16), (130, 16, 16),
          (130, 100, 24),    # 297 segments: workgroups whose four rows straddle two quarters of a block
          (130, 400, 8)]     # 1197 segments: two block parts per layer


@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_new_count_pass_matches_the_old_kernels(gpu, dims):
    ref = _both_paths(Sdfs.Sphere(1.0), [-1.5] * 3, [1.5] * 3, dims, clip=False)
    assert len(ref.Vertices) > 0 and ref.ActiveCells > 0


@pytest.mark.parametrize("dims", [(16, 16, 16), (72, 16, 520)], ids=lambda d: "x".join(map(str, d)))
def test_clip_to_bounds(gpu, dims):
    # a sphere larger than the box: every face of the grid is a surface once the faces are clipped
    ref = _both_paths(Sdfs.Sphere(2.5), [-1.5] * 3, [1.5] * 3, dims, clip=True)
    assert len(ref.Vertices) > 0


def test_case_13_sign_words(gpu):
    """A 3-D checkerboard block inside a sphere: every cell of the block has the sign word 0xA5 or 0x5A, the count pass's second
    counter (it decides whether k_resolve runs its dead-cell test)."""
    from sdfkit_amd.expr import select_lt
    n = 40

    def field(p):
        f = lambda t: MathF.Floor((t + 1.0) * (n / 2.0))          # the voxel index along one axis (sample points sit at index + 0.5)
        s = f(p.x) + f(p.y) + f(p.z)
        odd = s - MathF.Floor(s * 0.5) * 2.0                       # 0 or 1
        block = MathF.Max(MathF.Max(MathF.Abs(p.x), MathF.Abs(p.y)), MathF.Abs(p.z))
        sphere = MathF.Sqrt((p.x * p.x + p.y * p.y) + p.z * p.z) - 0.7
        return Vec4.of((0, 0, 0), select_lt(block, 0.3, (odd - 0.5) * (0.25 + p.x), sphere))

    ref = _both_paths(Sdf(field, False), [-1.0] * 3, [1.0] * 3, (n, n, n), clip=False)
    assert ref.ActiveCells > 1000
    _both_paths(Sdf(field, False), [-1.0] * 3, [1.0] * 3, (n, n, n), clip=False, elide=1)   # the sign-only sampler: the same bytes


@pytest.mark.parametrize("name", sorted(S.CATALOGUE))
def test_catalogue_scenes(gpu, name):
    _, sdf = S.CATALOGUE[name]()
    dims = (64, 64, 64) if name == "readme_repeat_xy" else (40, 36, 48)
    ref = _both_paths(sdf, [-2.8125] * 3, [2.8125] * 3, dims, clip=True)
    assert len(ref.Vertices) > 0


def test_other_pitch_keeps_the_old_kernels(gpu):
    """nz = 12: rows of 12 bytes, no 8-byte loads along z -- the job regroups the bytes into words as before, option or not"""
    _both_paths(Sdfs.Sphere(1.0), [-1.5] * 3, [1.5] * 3, (16, 16, 12), clip=False, expect_new=False)


def test_jobs_back_to_back_on_one_stream(gpu):
    """The new count pass ADDS into the block and quarter counts; k_resolve zeroes them behind their last reader and the next job with
    as many blocks takes the array over as it is.  One stream (no internal lanes), different scenes of one grid shape in a row: every
    mesh is the old path's."""
    mn, mx, dims = [-1.5] * 3, [1.5] * 3, (72, 20, 24)
    sdfs = [Sdfs.Sphere(1.0), Sdfs.Sphere(0.4), Sdfs.Box(0.8), Sdfs.Sphere(1.2)]
    with N.option(N.OPT_ELIDE_VOLUME, 0), N.option(N.OPT_LANES, 0), N.option(N.OPT_GRAPHS, 0):
        with N.option(N.OPT_COUNT_BYTES, 0):
            refs = [s.ToMesh(mn, mx, *dims, clipToBounds=False) for s in sdfs]
        with N.option(N.OPT_COUNT_BYTES, 1):
            for rnd in range(3):
                for s, ref in zip(sdfs, refs):
                    _assert_same(s.ToMesh(mn, mx, *dims, clipToBounds=False), ref, ("round", rnd))
    assert len({r.ActiveCells for r in refs}) == len(refs)      # (the jobs did leave different counts behind)


def test_default_configuration(gpu):
    """lanes, captured graphs and the product's volume-less default as they come: repeat calls (the third and later ones of a small grid
    are captured graphs, which keep the old kernels) give one mesh"""
    mn, mx, dims = [-1.5] * 3, [1.5] * 3, (64, 24, 32)
    with N.option(N.OPT_COUNT_BYTES, 0), N.option(N.OPT_ELIDE_VOLUME, 0):
        ref = Sdfs.Sphere(1.0).ToMesh(mn, mx, *dims)
    for rep in range(6):
        _assert_same(Sdfs.Sphere(1.0).ToMesh(mn, mx, *dims), ref, ("default", rep))
