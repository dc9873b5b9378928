"""Needle volumes through the product's block culling (SDFK_OPT_ELIDE_VOLUME = 2, the default of ToMesh) on the MI355X.

A needle volume is constant except for ONE voxel; the iso value is 0.  Every culler box that does not hold the needle is decided
"no surface" from the min/max pyramid sdfk_program_create_bound built (bind_volumes: the level offsets, one pyramid per channel
read, one block per slot; csrc/vol_pyramid.h's kernels) -- so a pyramid cell that misses the needle, or drops its NaN, deletes the
only geometry there is.  The grid is 264 x 260 x 256 over the volume's own box (above the captured-graph limit: the elided path
applies), the volumes are 33, 264 and 1056 voxels long in x: an 8-sample sub-box then spans 1, 8 and 32 voxels and the 128-sample
coarse box 16 times that, so every level up to the top decides boxes.  Per case: culled (mode 2) and sign-only (mode 1) equal
stored (mode 0) bit for bit, both culling kernels ran, and the stored mesh is where the numpy model of the sampled volume has its
sign changes.  On the CPU, before that: the model volume does read the needle, its intervals (tests/interval_model.py) leave
the needle's boxes undecided (check_not_vacuous says which those are) and decide more than half of all sub-boxes.

What this catches, found by making each change locally (none reads outside an allocation), building the library and running
this file once; every failure was "culled != stored", the culled mesh empty:
  k_vol_pyr_up skips child q == 7             36 cases: every finite, NaN and -inf needle at below_pow2 and, for 264 and 1056
                                              (Voxels[p]), at inner -- where the needle's level-1 cell is odd on all three axes --
                                              and test_needle_in_the_second_of_two_volumes[*-below_pow2]
  lev[] starts one level late                 10 cases, all at inner (264 nearest; 1056 nearest, and linear with NaN and -inf): the
                                              levels then overlap, and elsewhere the needle's cell is left alone or overwritten by
                                              a cell that holds the needle too (first, last, 2^k - 1 and 2^k all pass)
  channel 1's pyramid built from channel 0    test_needle_in_a_colour_channel[nearest-at_pow2] and [linear-at_pow2] ([*-last] pass:
                                              the last 8 samples of x are not a whole block and are never culled)
  __builtin_elementwise_minimum -> fminf      nothing here, and no mesh can: hi keeps the NaN and iv_whole makes the interval
  k_vol_pyr_base without the `bad` poison     unknown from it; a cell [c, inf] is still a bound of the clamped reads.  Both are
                                              caught where the pyramid itself is compared: tests/test_gpu_intervals.py
A +inf needle changes no sign (+inf > 0 like the background): those cases pin that nothing appears in any mode."""
import numpy as np
import pytest

from oracle import oracle as O
from sdfkit_amd import _native as N
from sdfkit_amd import Voxels
from sdfkit_amd.api import Sdf
from sdfkit_amd.expr import MathF, Vec4, trace_bound
from tests import interval_model as IM
from tests import test_interval_codegen as T
from tests import voxel_sdf_model as VM
from tests.test_gpu_elide_volume import _kernels_launched, _same_mesh
from tests.test_gpu_parity import assert_mesh_equal

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64

DIMS = (264, 260, 256)
MN, MX = (-1.0, -0.5, -0.25), (1.0, 0.5, 0.25)
SHAPES = [(33, 5, 3), (264, 5, 3), (1056, 5, 3)]
READS = {"nearest": VM.NEAREST, "linear": VM.LINEAR}
POSITIONS = ("first", "last", "below_pow2", "at_pow2", "inner")
# "inner": where a level-offset table that is wrong by one level overwrites the needle's cell, at the level the sub-boxes read, with a
# cell of constants (the levels of a pyramid lie back to back, so most shifted layouts leave a given cell alone or hand it a cell
# that holds the needle as well: 2^k - 1 and 2^k are such places for all three lengths)
INNER_X = {33: 9, 264: 99, 1056: 660}
# (background, needle): -1 in +1; the negated volume (the max side, and `<= iso` is the tie of the -1 background's boxes); non-finite
KINDS = {"neg": (1.0, -1.0), "negated": (-1.0, 1.0), "nan": (1.0, np.nan), "pinf": (1.0, np.inf), "ninf": (1.0, -np.inf)}
_AX = T.grid_axes(MN, MX, DIMS)


def _touching(n, op, axis, idx, upper_only=False):
    """(samples of the axis whose read takes voxel idx with a weight that is not zero -- upper_only: as the upper one of Sample's two
    voxels --, samples whose read touches it at all)"""
    d, mn = VM.vol_d((np.zeros(n, f32), None, MN, MX))[axis], f32(MN[axis])
    if op == VM.NEAREST:
        hit = VM.near_idx(VM.quot(_AX[axis], mn, d), n[axis]) == idx
        return hit, hit
    u = VM.lin_u(_AX[axis], f32(mn + f32(f32(0.5) * d)), d, n[axis])
    i0 = VM.lin_i0(u, n[axis])
    if n[axis] == 1:
        return i0 == idx, i0 == idx
    f = (u - i0.astype(f32)).astype(f32)
    return ((i0 == idx) & (f < 1) & (not upper_only)) | ((i0 + 1 == idx) & (f > 0)), (i0 == idx) | (i0 + 1 == idx)


def needle_index(n, op, position, kind="neg"):
    """The needle's voxel.  It has to be a voxel that some sample reads: with nx = k 264 a sample of Voxels[p] reads voxel i k + k / 2
    only (and Sample the two around it), so along x the position is moved to the nearest voxel that is read, without crossing the
    pyramid's cell boundary at 2^k: the first and the last voxel read; the last one at or below 2^k - 1, the first one at or above 2^k
    (2^k the largest power of two that is at most nx / 2: 16, 128, 512).  Sample shows a +inf voxel only where it is the upper one
    on every axis (as the lower one the lerp is inf + f (c - inf) = NaN, which the clamp to the corners' range turns into their
    minimum, the background): its first voxel is (1, 1, 1)."""
    upper = op == VM.LINEAR and kind == "pinf"
    read = [[i for i in range(n[a]) if _touching(n, op, a, i, upper)[0].any()] for a in range(3)]
    p2 = 1 << (int(n[0] // 2).bit_length() - 1)
    x = {"first": read[0][0], "last": read[0][-1], "below_pow2": max(i for i in read[0] if i <= p2 - 1),
         "at_pow2": min(i for i in read[0] if i >= p2), "inner": min(i for i in read[0] if i >= INNER_X[n[0]])}[position]
    # (with nx = 264 Sample's weights are 0 or 1 up to rounding: the voxels that show a +inf are where the rounding falls)
    assert upper or abs(x - {"first": 0, "last": n[0] - 1, "below_pow2": p2 - 1, "at_pow2": p2, "inner": INNER_X[n[0]]}[position]) <= max(1, n[0] // 264 // 2)
    # inside: y in the middle, z at its end -- with x = 2^k - 1 the needle's level-1 cell is then odd on all three axes, the last
    # of the eight children of its level-2 cell
    y, z = {"first": (read[1][0], read[2][0]), "last": (read[1][-1], read[2][-1])}.get(position, (n[1] // 2, n[2] - 1))
    assert y in read[1] and z in read[2] and (read[1][0], read[2][0]) == ((1, 1) if upper else (0, 0)) and (read[1][-1], read[2][-1]) == (n[1] - 1, n[2] - 1)
    return (x, y, z)


def needle_volume(n, idx, kind, channel=3):
    """the model volume (values, colours, Min, Max): the needle in the distance, or in colour channel `channel` of a volume whose
    distance and other colours are constant"""
    bg, needle = KINDS[kind]
    if channel == 3:
        vals = np.full(n, bg, f32)
        vals[idx] = needle
        return (vals, None, MN, MX)
    cols = np.full(n + (3,), 0.5, f32)
    cols[..., channel] = bg
    cols[idx + (channel,)] = needle
    return (np.full(n, 0.25, f32), cols, MN, MX)


class Case:
    """a program over needle volumes: the Sdf, and the model's (ops, out, volumes) of the same trace"""

    def __init__(self, fn, mvols, needle_slot, channel, op, idx, kind):
        self.vox = [Voxels(v[0], v[1], v[2], v[3]) for v in mvols]
        self.sdf = Sdf(lambda p: fn(p, self.vox), True)
        ops, out, bound = trace_bound(self.sdf.fn, True)
        assert all(b is v for b, v in zip(bound, self.vox)) and len(bound) == len(mvols)   # (slot order = order of first use)
        self.p = dict(name="needle", ops=ops, out=out, wc=1, vols=list(mvols))
        self.vol, self.channel, self.op, self.idx, self.bg = mvols[needle_slot], channel, op, idx, f32(KINDS[kind][0])
        self.finite = bool(np.isfinite(KINDS[kind][1]))


def _block(c):
    """per axis the slice of samples whose read touches the needle at all, one sample wider on each side: outside of it no index of
    a sample's read is the needle's on that axis, so the sample reads constants, and a read of constants c is c (Voxels[p] returns
    the voxel; Sample computes c + f (c - c) = c for a finite f, and the clamp to the corners' [c, c] keeps it)"""
    sl = []
    for a in range(3):
        hit = np.flatnonzero(_touching(c.vol[0].shape, c.op, a, c.idx[a])[1])
        assert len(hit) and np.all(np.diff(hit) == 1)
        sl.append(slice(max(int(hit[0]) - 1, 0), min(int(hit[-1]) + 2, DIMS[a])))
    return tuple(sl)


def model_block(c):
    """(slices, the model's sampled distance on them): the whole sampled volume is the background outside (see _block)"""
    sl = _block(c)
    shp = tuple(s.stop - s.start for s in sl)
    px = _AX[0][sl[0], None, None] + np.zeros(shp, f32)
    py = _AX[1][None, sl[1], None] + np.zeros(shp, f32)
    pz = _AX[2][None, None, sl[2]] + np.zeros(shp, f32)
    return sl, VM._eval(c.p["ops"], px, py, pz, c.p["vols"])[c.p["out"][3]]


def check_not_vacuous(c, sl, Wb):
    """the two conditions, on the CPU: the model's sampled volume reads the needle (a sample differs from the background); the model's
    intervals on the culler's boxes leave the needle's boxes undecided at iso 0 and decide more than half of all sub-boxes.  The
    needle's boxes: the sub-boxes and coarse boxes that hold a sample reading the needle and, for a finite needle, a sample that
    does not (a box of needle samples alone is rightly decided "no surface": Voxels[p] of the 33-voxel volumes has such boxes);
    there is at least one."""
    differs = ~T.bits_eq(Wb, np.full(Wb.shape, c.bg, f32))
    assert differs.any(), "no sample reads the needle"
    at = np.indices(Wb.shape).reshape(3, -1).T + np.array([s.start for s in sl])
    sub, coarse = T.culler_index_boxes(DIMS)
    held = 0
    for kind, idx, size in (("sub", sub, (8, 4, 4)), ("coarse", coarse, (128, 8, 8))):
        X, Y, Z = T.axis_boxes(_AX, idx)
        lo, hi = IM.interval(c.p["ops"], c.p["out"][3], X, Y, Z, c.p["vols"])
        with np.errstate(invalid="ignore"):
            decided = ~np.isnan(lo) & ((lo > 0) | (hi <= 0))
        b = at // np.array(size)
        ok = np.all(b < np.array(decided.shape), axis=1)   # (sub-boxes stop at the last whole block of x)
        boxes, inv = np.unique(b[ok], axis=0, return_inverse=True)
        inv = np.ravel(inv)
        count = lambda flag: np.bincount(inv, np.ravel(flag)[ok].astype(f64), len(boxes)) > 0
        has_needle, has_other = count(differs), count(~differs)
        # a box that reaches out of the block holds background samples too
        whole = np.prod(np.minimum((boxes + 1) * np.array(size), np.array(DIMS)) - boxes * np.array(size), axis=1)
        has_other |= np.bincount(inv, minlength=len(boxes)) < whole
        mine = boxes[has_needle & (has_other if c.finite else True)]
        held += len(mine)
        assert not decided[mine[:, 0], mine[:, 1], mine[:, 2]].any(), (kind, "the model decides one of the needle's boxes")
        if kind == "sub":
            assert decided.mean() > 0.5, decided.mean()
    assert held >= 1
    return held


def check_where_the_model_says(c, sl, Wb, mesh, geometry=True):
    """the stored mesh against the model's sampled volume: it has vertices exactly when the model has a cell with both signs
    (`> 0` and not), its finite vertices lie inside the hull of those cells, and for a finite needle every vertex is finite and
    within one voxel of the needle plus the grid step a vertex is interpolated over (a vertex lies on a grid edge with an end that
    reads the needle; that sample is at most one voxel from the needle's centre on every axis).  All in units of samples."""
    with np.errstate(invalid="ignore"):
        S = Wb > 0
    cells = [S[i:S.shape[0] - 1 + i, j:S.shape[1] - 1 + j, k:S.shape[2] - 1 + k] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    act = np.argwhere(np.any(cells, axis=0) & ~np.all(cells, axis=0)) + np.array([s.start for s in sl])
    V = np.asarray(mesh.Vertices, f32).reshape(-1, 3)
    assert (len(V) > 0) == (len(act) > 0), (len(V), len(act))
    if c.finite:
        assert (len(V) > 0 or not geometry) and np.isfinite(V).all()
    # (MarchingCubes puts sample i at Min + i (Max - Min) / (N - 1): back to sample indices, fractional along the edge of a vertex)
    ext = np.asarray(MX, f64) - np.asarray(MN, f64)
    fin = (V[np.isfinite(V).all(axis=1)].astype(f64) - np.asarray(MN, f64)) * (np.array(DIMS) - 1) / ext
    if len(fin):
        assert np.all(fin >= act.min(axis=0) - 1e-3) and np.all(fin <= act.max(axis=0) + 1 + 1e-3), (act.min(axis=0), act.max(axis=0) + 1, fin.min(0), fin.max(0))
    if c.finite:
        per_voxel = np.array(DIMS) / np.array(c.vol[0].shape)          # samples per voxel
        centre = (np.array(c.idx) + 0.5) * per_voxel - 0.5              # the needle's centre as a sample index
        assert np.all(np.abs(fin - centre) <= per_voxel + 1 + 1e-3), (centre, per_voxel, fin.min(0), fin.max(0))


def run_case(c, oracle=False, geometry=True):
    sl, Wb = model_block(c)
    check_not_vacuous(c, sl, Wb)
    meshes = {}
    for mode in (0, 2, 1):
        with N.option(N.OPT_ELIDE_VOLUME, mode):
            if mode == 2:
                meshes[mode], ran = _kernels_launched(lambda: c.sdf.ToMesh(MN, MX, *DIMS, clipToBounds=False))
                assert "sdfk_cull_blocks" in ran and "sdfk_eval_blocks" in ran, ran
            else:
                meshes[mode] = c.sdf.ToMesh(MN, MX, *DIMS, clipToBounds=False)
    assert _same_mesh(meshes[2], meshes[0]), ("culled != stored", len(meshes[2].Vertices), len(meshes[0].Vertices))
    assert _same_mesh(meshes[1], meshes[0]), ("sign-only != stored", len(meshes[1].Vertices), len(meshes[0].Vertices))
    check_where_the_model_says(c, sl, Wb, meshes[0], geometry)
    if oracle:   # the whole model volume, sampled point by point, under the oracle's sweep
        mv, mc = VM.sample(c.p["ops"], c.p["out"], True, MN, MX, *DIMS, c.p["vols"], clip=False)
        W = np.full(DIMS, c.bg, f32)
        W[sl] = Wb
        assert np.all(T.bits_eq(W, mv)), "the model volume is not the background outside the needle's block"
        assert_mesh_equal(meshes[0], O.march(mv, mc, MN, MX))


def _read(op, vox, p, channel=3):
    return p.x.b.voxel(op, vox, p, channel)


def _plain(op):
    if op == VM.NEAREST:
        return lambda p, vox: Vec4.of((1.0, 1.0, 1.0), vox[0][p])       # Voxels[p]
    return lambda p, vox: Vec4.of((1.0, 1.0, 1.0), vox[0].Sample(p))    # Voxels.Sample(p)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("position", POSITIONS)
@pytest.mark.parametrize("read", sorted(READS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_needle_mesh_survives_culling(gpu, shape, read, position, kind):
    op = READS[read]
    idx = needle_index(shape, op, position, kind)
    c = Case(_plain(op), [needle_volume(shape, idx, kind)], 0, 3, op, idx, kind)
    # one case per read kind also against the oracle's march of the whole model volume (17.5 M points in numpy: no other case)
    # Sample of the 1056-voxel volume gives every voxel the weight 1/2 along x (u = 4 i + 1.5): a finite needle moves the sampled
    # volume from +-1 to 0 = iso at most, the `<= iso` tie itself.  Whether a cell has both signs then hangs on the rounding of u
    # and on the clamped rows of y and z; the model says which, and the mesh must be empty where it has none
    run_case(c, oracle=(shape, position, kind) == ((264, 5, 3), "at_pow2", "neg"), geometry=(shape[0], read) != (1056, "linear"))


@pytest.mark.parametrize("position", ("last", "at_pow2"))
@pytest.mark.parametrize("read", sorted(READS))
def test_needle_in_a_colour_channel(gpu, read, position):
    """w reads colour channel 1 of a coloured volume, the needle sits in that channel only (the distance and the other colours are
    constant), and the mesh's colour reads channels 0 and 2: three pyramids of one slot, built from the stride-3 source, each at its
    own offset"""
    op, shape = READS[read], (264, 5, 3)
    idx = needle_index(shape, op, position)

    def fn(p, vox):
        return Vec4(_read(op, vox[0], p, 0), 1.0, _read(op, vox[0], p, 2), _read(op, vox[0], p, 1))
    run_case(Case(fn, [needle_volume(shape, idx, "neg", channel=1)], 0, 1, op, idx, "neg"))


@pytest.mark.parametrize("position", ("last", "below_pow2"))
@pytest.mark.parametrize("read", sorted(READS))
def test_needle_in_the_second_of_two_volumes(gpu, read, position):
    """w = min(a[p], b[p]): slot 0 is the larger volume (1056 x 5 x 3, constant), the needle is in slot 1 (33 x 5 x 3) only: one block
    per slot, the second one behind the first one's values and pyramid"""
    op, shape = READS[read], (33, 5, 3)
    idx = needle_index(shape, op, position)

    def fn(p, vox):
        return Vec4.of((1.0, 1.0, 1.0), MathF.Min(_read(op, vox[0], p), _read(op, vox[1], p)))
    run_case(Case(fn, [(np.full((1056, 5, 3), 1.0, f32), None, MN, MX), needle_volume(shape, idx, "neg")], 1, 3, op, idx, "neg"))
