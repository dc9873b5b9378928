"""CPU side of the Voxels.Redistance stress cases (tests/redistance_cases.py): what each case is for is asserted on the numpy model
(tests/redistance_model.py), the g++ host solver built from csrc/redistance.h equals the model on every one, and a numpy
emulation of the DEVICE LAYOUT of csrc/lib_redistance.hip (two buffers, two flag arrays, the sweep rule of k_rd_sweep, the
32-sweep batches of the host loop) shows that the cases have teeth: broken so that a swept but unchanged tile does not rewrite
its output buffer, it is caught by the re-activation cases and NOT by the sphere the first GPU tests ran -- none of their inputs
ever sweeps a tile again after it went idle.

The re-activation conditions of the cases, across them: a tile swept again after an odd gap, after an even gap, after a gap of 8
sweeps or more, and a woken tile that changes in the very sweep that wakes it.  The last is rare: a sweep reads face neighbours
only, so the change has to come in at a tile corner from a tile that is no face neighbour, in the one sweep in which no face
neighbour changed; the waves of point insides in a field of ones never do that, and the case that does (wake_at_once_16x24x1)
was found by a search over random sign patterns.

What the broken emulation stands for.  A tile's last unchanged sweep before it goes idle is the only write the schedule needs
for a LATER wake-up and for nothing else; leaving it out is what any of these real mistakes amounts to at the moment of the
wake-up: a kernel that skips the store of an unchanged tile, a tile that wakes on the wrong buffer parity after an odd gap
(it reads the buffer it did not write last), or a buffer left stale because the idle path was given the copy to do and does not
do it.  The emulation restores the tile's old output after the sweep, since within the sweep nothing knows that the tile is
about to go idle: it is a mutation of the invariant, not the sweep rule of k_rd_sweep with a switch.  It is caught by
wake_17x41x9 and wake_at_once_16x24x1 and their banded variants, and not by wake_16x64x1."""
import numpy as np
import pytest

from tests import redistance_cases as RC
from tests import redistance_model as M

f32 = np.float32
INF = float("inf")
TILE = M.TILE
BATCH = 32   # kBatch of csrc/lib_redistance.hip


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


_model_cache = {}


def model(c):
    if c.name not in _model_cache:
        _model_cache[c.name] = RC.model(c)
    return _model_cache[c.name]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return M.build_host_solver(tmp_path_factory.mktemp("redistance_cases"))


def _host_equals_model(exe, tmp_path, cases):
    for c in cases:
        got, gst = M.host_solve(exe, c.values, RC.cell_sizes(c), c.iso, c.band, tmp_path, tag=c.name)
        want, wst = model(c)
        bad = np.argwhere(_bits(got) != _bits(want))
        assert len(bad) == 0, (c.name, len(bad), bad[:4], got[tuple(bad[:4].T)], want[tuple(bad[:4].T)])
        assert gst == {k: wst[k] for k in gst}, (c.name, gst, wst)


# ---- the device layout in numpy ------------------------------------------------------------------------------------------------
def _box(tile, shape):
    return tuple(slice(int(i) * TILE, min((int(i) + 1) * TILE, n)) for i, n in zip(tile, shape))


def emulate_device(values, h, iso=0.0, band=INF, skip_unchanged_write=None):
    """csrc/lib_redistance.hip step by step, with the model's arithmetic: k_rd_front writes T0 (frozen: sign bit set) into BOTH
    buffers and the tiles' sweep-0 flags; sweep k reads buffer (k - 1) & 1 and flag array (k - 1) & 1 and writes the others, a
    tile only if it or a face neighbour is flagged (an idle tile clears its flag and writes nothing else); a sweep k > last + 1
    does nothing; the host queues 32 sweeps, then reads `last`; k_rd_finish reads buffer 0.
    skip_unchanged_write: the bug the re-activation cases are for -- a swept tile that changed nothing leaves its output alone,
    "always", or only in its last sweep before it goes idle while the solve goes on ("going idle": exactly the tiles on which
    the two buffers have to agree for a later wake-up; every other unchanged tile is read again in the next sweep, by itself)."""
    values = np.asarray(values, f32)
    band = f32(band)
    out, frozen, T0 = M.front(values, h, iso)
    with np.errstate(all="ignore"):
        t = [np.where(frozen, -T0, T0).astype(f32) for _ in range(2)]
    tiles = tuple((n + TILE - 1) // TILE for n in values.shape)
    flag = [M._tiles_of(frozen), np.zeros(tiles, bool)]   # (flag[1] is uninitialised on the device: every tile writes it in sweep 1)
    assert flag[0].shape == tiles
    last = 0 if frozen.any() else -1
    tile_sweeps = queued = 0
    while True:
        for _ in range(BATCH):
            queued += 1
            k = queued
            if last < k - 1:
                continue
            t_in, t_out, f_in, f_out = t[(k - 1) & 1], t[k & 1], flag[(k - 1) & 1], flag[k & 1]
            act = M._dilate6(f_in)
            new = M.sweep(np.abs(t_in), np.signbit(t_in), h, band)
            before = t_out.copy() if skip_unchanged_write == "going idle" else None
            for tile in np.ndindex(*tiles):
                if not act[tile]:
                    f_out[tile] = False
                    continue
                box = _box(tile, values.shape)
                changed = bool((new[box] < np.abs(t_in[box])).any())
                if changed or skip_unchanged_write != "always":
                    t_out[box] = np.where(np.signbit(t_in[box]), t_in[box], new[box])
                f_out[tile] = changed
                if changed:
                    last = max(last, k)
                tile_sweeps += 1
            if before is not None and f_out.any():   # (the solve goes on)
                for tile in np.argwhere(act & ~M._dilate6(f_out)):
                    t_out[_box(tile, values.shape)] = before[_box(tile, values.shape)]
        if last < queued:
            break
        if queued > BATCH * (2 + sum(values.shape) // BATCH):   # (twice what any case here needs)
            return None, {"sweeps": None, "tile_sweeps": tile_sweeps}   # the broken schedule may never settle: two buffers that disagree
    T = np.abs(t[0])
    m = np.where(T < band, T, band).astype(f32)
    res = np.where(out, m, -m).astype(f32)
    return res, {"sweeps": last + 1, "tile_sweeps": tile_sweeps, "front": int(frozen.sum()), "clamped": int((T > band).sum())}


def _emulation_differs(c, **kw):
    got, gst = emulate_device(c.values, RC.cell_sizes(c), c.iso, c.band, **kw)
    want, wst = model(c)
    return got is None or bool(np.any(_bits(got) != _bits(want))) or gst != wst


def _sphere32():
    v, _, _ = M.sphere_inputs(32, "b")
    return RC.Case("sphere32b", v, [-1.5] * 3, [1.5] * 3, 0.0, INF)


def test_emulation_of_the_device_layout_equals_model():
    for c in RC.all_cases():
        assert not _emulation_differs(c), c.name


def test_unwritten_unchanged_tiles_are_caught_by_the_new_cases_only():
    """Skipped in EVERY unchanged sweep, the write is missed at once: the tile reads its own stale values two sweeps later, 'changes'
    again, and the solve never settles -- on any input, the sphere of the first GPU tests included.  Skipped only where the
    contract needs it for a wake-up (the last sweep before a tile goes idle), it passes the sphere and fails the new cases."""
    new = RC.reactivation_cases() + RC.reactivation_cases(banded=True)
    caught = [c.name for c in new if _emulation_differs(c, skip_unchanged_write="going idle")]
    print("caught by", caught)
    assert {"wake_17x41x9", "wake_17x41x9_banded"} <= set(caught) and all(_emulation_differs(c, skip_unchanged_write="always") for c in new)
    # what the first GPU tests could not see: the sphere never sweeps an idle tile again
    c = _sphere32()
    assert not M.idle_gaps(M.schedule_history(c.values, RC.cell_sizes(c)))
    assert not _emulation_differs(c, skip_unchanged_write="going idle")
    assert emulate_device(c.values, RC.cell_sizes(c), skip_unchanged_write="always")[1]["sweeps"] is None   # (never settles)


def test_earlier_inputs_never_wake_an_idle_tile():
    """The inputs of tests/test_gpu_redistance.py that the model replays quickly: every tile's sweeps are one contiguous run."""
    v = np.random.default_rng(0).uniform(-1, 1, (17, 17, 17)).astype(f32)
    assert not M.idle_gaps(M.schedule_history(v, M.cell_sizes([0] * 3, [1] * 3, v.shape)))
    v = np.ones((11, 11, 11), f32)
    v[5, 5, 5] = -1.0
    assert not M.idle_gaps(M.schedule_history(v, M.cell_sizes([0] * 3, [1.1, 2.2, 3.3], v.shape)))


# ---- 1. / 2. the schedule helpers and the re-activation cases --------------------------------------------------------------------
def test_idle_gaps_of_a_hand_made_history():
    on, off = np.ones((1, 1, 1), bool), np.zeros((1, 1, 1), bool)
    assert M.idle_gaps([on, on, on]) == set() and M.idle_gaps([]) == set()
    assert M.idle_gaps([off, on, off, off]) == set()                      # not swept yet / no longer swept: no gap
    assert M.idle_gaps([on, off, on, off, off, off, on, on]) == {1, 3}
    two = [np.array([a, b]).reshape(2, 1, 1) for a, b in [(1, 1), (0, 1), (0, 0), (1, 0), (0, 1)]]
    assert M.idle_gaps(two) == {2} and sorted(M.idle_runs(two)) == [((0, 0, 0), 1, 2), ((1, 0, 0), 2, 2)]


def test_reactivation_conditions():
    gaps_all, woken_changes, wakes_changing_at_once = set(), 0, 0
    for banded in (False, True):
        for c, (_, shape, _, _, sweeps, gaps, _) in zip(RC.reactivation_cases(banded), RC.REACTIVATION_SPECS):
            assert c.values.shape == shape
            _, st = model(c)
            swept, changed = M.schedule_history(c.values, RC.cell_sizes(c), c.iso, c.band, changes=True)
            assert len(swept) == st["sweeps"] and sum(int(s.sum()) for s in swept) == st["tile_sweeps"]
            got = M.idle_gaps(swept)
            print(c.name, st, "idle gaps", sorted(got))
            if banded:
                assert got and st["clamped"] > 0   # the band cuts the solve, and the late wave still arrives
            else:
                assert st["sweeps"] == sweeps and got == gaps
            gaps_all |= got
            for tile, first, g in M.idle_runs(swept):
                k = first + g                       # the sweep that wakes the tile; it stays swept until the next gap or the end
                end = k
                while end < len(swept) and swept[end][tile]:
                    end += 1
                woken_changes += any(changed[i][tile] for i in range(k, end))
                wakes_changing_at_once += bool(changed[k][tile])
    print("gaps", sorted(gaps_all), "woken tiles that change", woken_changes, "of them in the waking sweep", wakes_changing_at_once)
    assert any(g % 2 == 1 for g in gaps_all) and any(g % 2 == 0 for g in gaps_all) and any(g >= 8 for g in gaps_all)
    assert woken_changes > 0 and wakes_changing_at_once > 0
    # the tile that changes in its waking sweep: the one the case names, unbanded and banded
    for c in (RC.reactivation_cases()[2], RC.reactivation_cases(banded=True)[2]):
        swept, changed = M.schedule_history(c.values, RC.cell_sizes(c), c.iso, c.band, changes=True)
        assert ((0, 0, 0), 5, 1) in M.idle_runs(swept) and swept[4][0, 0, 0] and not swept[5][0, 0, 0] and changed[6][0, 0, 0]
        assert not changed[4][0, 1, 0] and not changed[4][1, 0, 0] and changed[4][1, 1, 0]   # two sweeps before: the diagonal tile only
        assert changed[5][0, 1, 0] or changed[5][1, 0, 0]                                  # then a face neighbour, at the corner


def test_reactivation_cases_match_host_solver(host_exe, tmp_path):
    _host_equals_model(host_exe, tmp_path, RC.reactivation_cases() + RC.reactivation_cases(banded=True))


# ---- 3. batch edges ------------------------------------------------------------------------------------------------------------
def test_lines_reach_the_fixed_point_at_the_batch_edges(host_exe, tmp_path):
    cases = RC.batch_cases()
    assert len(cases) == 18
    for c in cases:
        n = c.values.size
        assert np.array_equal(RC.cell_sizes(c), np.ones(3, f32)) and model(c)[1]["sweeps"] == n - 1, c.name
    assert {model(c)[1]["sweeps"] for c in cases} == {BATCH, BATCH + 1, BATCH + 2, 2 * BATCH, 2 * BATCH + 1, 2 * BATCH + 2}
    _host_equals_model(host_exe, tmp_path, cases)


# ---- 4. thin and ragged shapes ---------------------------------------------------------------------------------------------------
def test_thin_shapes_match_host_solver(host_exe, tmp_path):
    cases = RC.thin_cases()
    assert [c.values.shape for c in cases[:len(RC.THIN_SHAPES)]] == RC.THIN_SHAPES and max(c.values.size for c in cases) == 16 ** 3
    for c in cases[-2:]:   # one inside voxel on either side of the tile corner: its seven front voxels lie in four tiles
        frozen = M.front(c.values, RC.cell_sizes(c))[1]
        assert frozen.sum() == 7 and M._tiles_of(frozen).sum() == 4
    _host_equals_model(host_exe, tmp_path, cases)


# ---- 5. extremes ---------------------------------------------------------------------------------------------------------------
def test_extreme_cases_are_what_they_claim_and_match_host_solver(host_exe, tmp_path):
    cases = {c.name: c for c in RC.extreme_cases()}
    tiny = np.finfo(f32).tiny
    res, st = model(cases["box_1e-37"])
    denormal = int(((res != 0) & (np.abs(res) < tiny)).sum())
    print("denormal results", denormal, "cell sizes", RC.cell_sizes(cases["box_1e-37"]))
    assert denormal >= 100 and 0 < RC.cell_sizes(cases["box_1e-37"])[0] < tiny   # (DX only: DY, DZ are 2e-38 and 2.7e-38)
    for name in ("box_1e30_1e-30_1", "box_3e38", "values_3e38", "values_1e-40"):
        res, st = model(cases[name])
        assert np.all(np.isfinite(res)) and st["front"] > 400 and st["sweeps"] >= 8, name
    assert np.all(np.abs(cases["values_1e-40"].values) < tiny) and np.abs(cases["values_3e38"].values).max() > 2.9e38
    c = cases["values_1e-44_and_3e38"]
    res, st = model(c)
    _, frozen, T0 = M.front(c.values, RC.cell_sizes(c))
    zeros, negative = int((res == 0).sum()), int(((res == 0) & np.signbit(res)).sum())
    print("T0 == 0:", int((T0 == 0).sum()), "zero results", zeros, "of them -0.0", negative)
    assert (c.values == 0).sum() == 0 and (T0 == 0).sum() >= 100 and zeros >= 100 and 50 <= negative < zeros
    for name in ("iso_2.9e38", "iso_-2.9e38"):
        c = cases[name]
        res, st = model(c)
        assert abs(c.iso) > 2.8e38 and (c.values > c.iso).any() and (c.values < c.iso).any() and st["front"] > 400 and np.all(np.isfinite(res))
    _host_equals_model(host_exe, tmp_path, cases.values())


# ---- 6. band edges -------------------------------------------------------------------------------------------------------------
def test_band_edges(host_exe, tmp_path):
    full, _ = model(RC.line(40, 0))
    reached = set(np.abs(full).ravel().tolist())
    assert {1.5, 2.5} <= reached and 3.0 not in reached and min(reached) == 0.5
    for band, clamped in RC.BAND_LINE.items():
        res, st = model(RC.line(40, 0, band=band))
        assert st["clamped"] == clamped, (band, st)
        assert np.array_equal(_bits(res), _bits(np.where(np.abs(full) < f32(band), full, np.copysign(f32(band), full))))
    cases = RC.band_cases()
    for c in cases:
        if c.name.endswith("_between"):   # the band lies between two values the unbanded solve reaches, where it reaches any
            free, _ = model(c._replace(name=c.name + "_unbanded", band=INF))
            mag = np.abs(free)
            assert not (mag == f32(c.band)).any(), c.name
            if c.name.startswith("wake") or c.values.size > 100:
                assert (mag < c.band).any() and (mag > c.band).any() and model(c)[1]["clamped"] > 0, c.name
        elif c.name.endswith("_band0"):
            res, st = model(c)
            assert st["clamped"] == int((np.abs(model(c._replace(name=c.name + "_unbanded", band=INF))[0]) > 0).sum())
            assert np.all(res == 0)
    _host_equals_model(host_exe, tmp_path, cases)


# ---- 9. the model's refusal -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mx", [(1, -1, 1), (1, 0, 1), (np.nan, 1, 1), (1, 1, np.inf), (-np.inf, 1, 1)])
def test_model_refuses_cell_sizes_that_are_not_positive_and_finite(mx):
    v = np.random.default_rng(3).uniform(-1, 1, (9, 10, 11)).astype(f32)
    with np.errstate(all="ignore"):
        h = M.cell_sizes([0, 0, 0], mx, v.shape)
    assert not (np.all(np.isfinite(h)) and np.all(h > 0))
    with pytest.raises(ValueError, match="cell sizes"):
        M.redistance(v, h)
    M.redistance(v, M.cell_sizes([0, 0, 0], [1, 1, 1], v.shape))


def test_all_cases_have_distinct_names():
    names = [c.name for c in RC.all_cases()]
    assert len(names) == len(set(names))
