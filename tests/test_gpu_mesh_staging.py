"""What the host staging of the triangle-mesh entry points (csrc/device_stage.h under lib_trimesh*.hip) must keep, in one place:
an optional output left null changes no other output; a compacted output is written up to its count and no further; a null
positions3 means the handle's own vertices; a host form writes the bytes its device form writes; the buffers a handle adopts
(labels, adjacency, sampling weights) outlive the call that made them.  Through the ctypes table of sdfkit_amd/_native.py.

The mesh is a cube and a disjoint tetrahedron with colours, in two forms.  SOUP: every triangle with three vertices of its own
(16 triangles, 48 vertices, 12 distinct positions) -- duplicates for the weld, a kept count below nv.  INDEXED: the same
triangles over the 12 positions -- by index two components, for components / topology / select.  (By index the soup is 16
components: connectivity is by index, so one mesh cannot both have duplicates everywhere and two components.)  Staging goes wrong
in the pointer and length bookkeeping, not at scale: everything is compared byte for byte, canaries included."""
import ctypes as C

import numpy as np
import pytest

from sdfkit_amd import _native as N

pytestmark = pytest.mark.gpu
f32, i32, i64, u32, u8 = np.float32, np.int32, np.int64, np.uint32, np.uint8
CANARY = 7


def _mesh():
    cube = np.array([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)], f32)
    ct = np.array([(0, 2, 1), (1, 2, 3), (4, 5, 6), (5, 7, 6), (0, 1, 4), (1, 5, 4), (2, 6, 3), (3, 6, 7), (0, 4, 2), (2, 4, 6), (1, 3, 5), (3, 7, 5)], i32)
    tet = np.array([(3, 0, 0), (4, 0, 0), (3, 1, 0), (3, 0, 1)], f32)
    tt = np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], i32) + 8
    V, T = np.concatenate([cube, tet]), np.concatenate([ct, tt])
    cols = np.random.default_rng(5).random((12, 3)).astype(f32)
    return {"indexed": (V, T.reshape(-1).copy(), cols),
            "soup": (np.ascontiguousarray(V[T].reshape(-1, 3)), np.arange(48, dtype=i32), np.ascontiguousarray(cols[T].reshape(-1, 3)))}


MESH = _mesh()
QUERIES = np.array([(0.5, 0.5, 0.5), (2.0, 0.2, 0.1), (3.1, 0.1, 0.1), (-1.0, 2.0, 0.5), (3.5, 3.0, -2.0)], f32)


def _vp(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def handles(gpu):
    L, hs = N.lib(), {}
    for name, (V, T, cols) in MESH.items():
        h = C.c_void_p()
        N.check(L.sdfk_trimesh_create(_vp(V), len(V), _vp(T), len(T), _vp(cols), C.byref(h)))
        hs[name] = h
    yield hs
    for h in hs.values():
        L.sdfk_trimesh_free(h)


class _Scalars:
    """int64 outputs of a call: counts by reference and stats arrays."""

    def __init__(self, *lengths):   # 0: an int64 by reference; k > 0: int64[k]
        self.v = [C.c_int64(-CANARY) if k == 0 else (C.c_int64 * k)(*[-CANARY] * k) for k in lengths]

    def args(self):
        return [C.byref(x) if isinstance(x, C.c_int64) else x for x in self.v]

    def values(self):
        return [x.value if isinstance(x, C.c_int64) else list(x) for x in self.v]


_TORCH = {f32: "float32", i32: "int32", u32: "int32", u8: "uint8", i64: "int64"}


def _device_array(a):
    """A numpy array as a torch tensor on the device (u32 as its int32 bits)."""
    import torch
    t = torch.from_numpy(a.view(i32) if a.dtype == u32 else a).to(torch.device("cuda", N._inited_device or 0))
    return t


def _call(name, pre, outs, scalars, only=None, device=False):
    """L.<name>(*pre, *outputs, *scalars) or its _device form.  outs: (dtype, shape) per optional output array, each filled with
    the canary (or (dtype, array): an array the call updates in place, which starts as a copy of that one); all are passed, or
    the one at index `only` and null for the rest.  pre: leading arguments; a numpy array among
    them is passed by pointer, from device memory for the device form.  -> ([array or None per output], scalar values)."""
    L = N.lib()
    hold, args, back = [], [], []
    if device:
        import torch
        N.bind_torch_stream()
    for p in pre:
        if isinstance(p, np.ndarray):
            hold.append(_device_array(p) if device else p)
            args.append(C.c_void_p(hold[-1].data_ptr()) if device else _vp(p))
        else:
            args.append(p)
    for k, (dt, shape) in enumerate(outs):
        if only is not None and k != only:
            args.append(None)
            back.append(None)
            continue
        a = np.array(shape, dt) if isinstance(shape, np.ndarray) else np.full(shape, CANARY, dt)
        hold.append(_device_array(a) if device else a)
        args.append(C.c_void_p(hold[-1].data_ptr()) if device else _vp(a))
        back.append(hold[-1])
    if device:
        torch.cuda.synchronize()
    N.check(getattr(L, name + ("_device" if device else ""))(*args, *scalars.args()))
    if device:
        torch.cuda.synchronize()
        back = [None if b is None else b.cpu().numpy().view(outs[k][0]) for k, b in enumerate(back)]
    return back, scalars.values()


def _entries(handles):
    """name -> (pre, outs, scalar lengths) of every entry point with optional outputs, on the mesh that exercises it."""
    soup, indexed = handles["soup"], handles["indexed"]
    n = len(QUERIES)
    return {
        "sdfk_trimesh_closest": ([soup, QUERIES, n], [(i32, (n,)), (f32, (n,)), (f32, (n, 3))], ()),
        "sdfk_trimesh_sample": ([soup, 33, C.c_uint64(2024), 1], [(f32, (33, 3)), (f32, (33, 3)), (f32, (33, 3)), (i32, (33,)), (f32, (33, 3))], (2,)),
        "sdfk_trimesh_components": ([indexed], [(i32, (12,)), (i32, (16,))], (0, 4)),
        "sdfk_trimesh_adjacency": ([indexed], [(u32, (13,)), (u32, (96,)), (u8, (12,))], (0,)),
        "sdfk_trimesh_select": ([indexed, np.array([0, 1], u8)], [(i32, (12,)), (i32, (16,)), (i32, (48,)), (f32, (12, 3)), (f32, (12, 3))], (0, 0)),
        "sdfk_trimesh_weld": ([soup, C.c_float(0.0), 0], [(i32, (48,)), (i32, (49,)), (i32, (17,)), (i32, (51,)), (f32, (49, 3)), (f32, (49, 3))], (0, 0, 4)),
    }


def _scalars_of(lengths):
    return _Scalars(*lengths)


@pytest.mark.parametrize("name", ["sdfk_trimesh_closest", "sdfk_trimesh_sample", "sdfk_trimesh_components", "sdfk_trimesh_adjacency",
                                  "sdfk_trimesh_select", "sdfk_trimesh_weld"])
def test_an_optional_output_alone_equals_it_among_all(handles, name):
    pre, outs, lengths = _entries(handles)[name]
    full, counts = _call(name, pre, outs, _scalars_of(lengths))
    assert not any(np.all(a == CANARY) for a in full), name          # (every output was written)
    for k in range(len(outs)):
        lone, lone_counts = _call(name, pre, outs, _scalars_of(lengths), only=k)
        assert lone[k].tobytes() == full[k].tobytes(), (name, k)
        assert lone_counts == counts, (name, k)
    none, none_counts = _call(name, pre, outs, _scalars_of(lengths), only=-1)   # (nothing asked for: not an error, the same counts)
    assert none_counts == counts, name


def test_topology_census_and_rows_each_alone(handles):
    L, h = N.lib(), handles["indexed"]

    def run(with_census, with_rows):
        census, rows = (C.c_int64 * 8)(*[-CANARY] * 8), np.full((2, 8), CANARY, i64)
        N.check(L.sdfk_trimesh_topology(h, census if with_census else None, _vp(rows) if with_rows else None, 2))
        return list(census), rows

    census, rows = run(True, True)
    assert census[0] == 2 and census[1] == 12 and not np.any(rows == CANARY)
    lone_census, untouched_rows = run(True, False)
    untouched_census, lone_rows = run(False, True)
    assert lone_census == census and np.all(untouched_rows == CANARY)
    assert lone_rows.tobytes() == rows.tobytes() and untouched_census == [-CANARY] * 8


def test_compacted_outputs_stop_at_the_kept_counts(handles):
    L = N.lib()
    # select: the tetrahedron alone (component 1: labels ascend with the least vertex) -- 4 of 12 vertices, 4 of 16 triangles
    pre, outs, lengths = _entries(handles)["sdfk_trimesh_select"]
    (vi, ti, tr, vs, cs), (kv, kt) = _call("sdfk_trimesh_select", pre, outs, _scalars_of(lengths))
    assert (kv, kt) == (4, 4)
    assert list(vi[:4]) == [8, 9, 10, 11] and list(ti[:4]) == [12, 13, 14, 15] and tr[:12].max() == 3
    assert np.array_equal(vs[:4], MESH["indexed"][0][8:]) and np.array_equal(cs[:4], MESH["indexed"][2][8:])
    for a, k in ((vi, kv), (ti, kt), (tr, 3 * kt), (vs, kv), (cs, kv)):
        assert np.all(a[k:] == CANARY) and len(a) > k
    # weld, exact mode: 48 -> 12 vertices; every triangle stays, so those arrays are one row longer than the mesh
    pre, outs, lengths = _entries(handles)["sdfk_trimesh_weld"]
    (vm, vi, ti, tr, vs, cs), (kv, kt, st) = _call("sdfk_trimesh_weld", pre, outs, _scalars_of(lengths))
    assert (kv, kt, st[:3]) == (12, 16, [36, 0, 0])
    assert vm.min() == 0 and vm.max() == 11 and len(np.unique(vm)) == 12          # (written whole: it is not compacted)
    for a, k in ((vi, kv), (ti, kt), (tr, 3 * kt), (vs, kv), (cs, kv)):
        assert np.all(a[k:] == CANARY) and len(a) > k
    assert np.array_equal(vs[:kv], MESH["soup"][0][vi[:kv]]) and np.array_equal(cs[:kv], MESH["soup"][2][vi[:kv]])
    # topology: room for one row of two
    census, rows = (C.c_int64 * 8)(), np.full((2, 8), CANARY, i64)
    N.check(L.sdfk_trimesh_topology(handles["indexed"], census, _vp(rows), 1))
    assert census[0] == 2 and list(rows[0, :3]) == [12, 8, 18] and np.all(rows[1] == CANARY)   # (the cube's row; the second row stays)


def test_null_positions_are_the_handles_own_vertices(handles):
    L = N.lib()
    for name in ("soup", "indexed"):
        V = MESH[name][0]
        for flags in (0, 1):
            own, given = np.full(V.shape, CANARY, f32), np.full(V.shape, CANARY, f32)
            N.check(L.sdfk_trimesh_vertex_normals(handles[name], None, flags, _vp(own)))
            N.check(L.sdfk_trimesh_vertex_normals(handles[name], _vp(V), flags, _vp(given)))
            assert own.tobytes() == given.tobytes() and not np.any(own == CANARY), (name, flags)


def test_host_forms_write_what_device_forms_write(handles):
    entries = _entries(handles)
    V = MESH["indexed"][0]
    fl = C.c_float
    entries.update({   # (iterations 0, 1, 3 and a Taubin pair: the copy alone, one step without a temporary, the ping-pong both ways)
        "smooth 0": ("sdfk_trimesh_smooth", [handles["indexed"], 0, fl(0.5), fl(0.0), 0], [(f32, V.shape)], ()),
        "smooth 1": ("sdfk_trimesh_smooth", [handles["indexed"], 1, fl(0.5), fl(0.0), 0], [(f32, V.shape)], ()),
        "smooth 3": ("sdfk_trimesh_smooth", [handles["indexed"], 3, fl(0.5), fl(0.0), 1], [(f32, V.shape)], ()),
        "smooth taubin": ("sdfk_trimesh_smooth", [handles["soup"], 1, fl(0.5), fl(-0.53), 0], [(f32, (48, 3))], ()),
        "normals own": ("sdfk_trimesh_vertex_normals", [handles["indexed"], None, 0], [(f32, V.shape)], ()),
        "normals given": ("sdfk_trimesh_vertex_normals", [handles["indexed"], np.ascontiguousarray(V[::-1] * f32(1.5)), 1], [(f32, V.shape)], ()),
    })
    for what, entry in entries.items():
        name, pre, outs, lengths = entry if len(entry) == 4 else (what,) + entry
        host, host_counts = _call(name, pre, outs, _scalars_of(lengths))
        dev, dev_counts = _call(name, pre, outs, _scalars_of(lengths), device=True)
        assert host_counts == dev_counts, what
        for k, (a, b) in enumerate(zip(host, dev)):
            assert a.tobytes() == b.tobytes(), (what, k)     # (canaries beyond the counts included)
        assert not any(np.all(a == CANARY) for a in host), what


def test_a_second_call_finds_what_the_first_left_on_the_handle(gpu):
    L = N.lib()
    V, T, cols = MESH["indexed"]
    h = C.c_void_p()
    N.check(L.sdfk_trimesh_create(_vp(V), len(V), _vp(T), len(T), _vp(cols), C.byref(h)))
    handles = {"indexed": h, "soup": h}

    def once():
        census, rows = (C.c_int64 * 8)(), np.full((2, 8), CANARY, i64)
        N.check(L.sdfk_trimesh_topology(h, census, _vp(rows), 2))                 # makes the labels and the weights
        _, outs, lengths = _entries(handles)["sdfk_trimesh_adjacency"]
        adjacency = _call("sdfk_trimesh_adjacency", [h], outs, _scalars_of(lengths))   # makes the adjacency
        pre, outs, lengths = _entries(handles)["sdfk_trimesh_sample"]
        sample = _call("sdfk_trimesh_sample", pre, outs, _scalars_of(lengths))         # reads the weights
        return [list(census), rows.tobytes()] + [a.tobytes() for a in adjacency[0] + sample[0]] + adjacency[1] + sample[1]

    first, second = once(), once()
    assert first == second
    L.sdfk_trimesh_free(h)
