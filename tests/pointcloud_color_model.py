"""A numpy model of per-point colours in the point-cloud pipeline (include/sdfkit_hip.h, "Point clouds: colours"), the yardstick of
sdfkit_amd.points.KdTree.SampleColors / ToVoxels(colors=) / VoxelDownsample(colors=) (csrc/lib_pointcloud.hip,
csrc/lib_points_filter.hip, csrc/points_color.h).  Not a test module.

Neighbours come from tests/points_knn_model.knn, the cut-off and the cell centres from tests/pointcloud_model.py, the groups and
the chunked sums from tests/points_filter_model.py.  Everything after them is float64 from the float32 inputs, one numpy operation
per operation of points_color.h, in its order (numpy's float64 + - * / are correctly rounded and never fused), and one rounding to
float32 per result -- so the library's results equal these bit for bit.
"""
import numpy as np

from tests import pointcloud_model as PC
from tests import points_filter_model as FM
from tests import points_knn_model as KM

f32 = np.float32
f64 = np.float64


def _colors(colors, n):
    c = np.ascontiguousarray(np.asarray(colors, f32).reshape(-1, 3))
    assert len(c) == n
    return c


def blend_rows(colors, d2, found, k, max_distance, idx):
    """Steps 2-5 of sdfk_points_blend_colors for given knn rows: idx (m, k) (-1: none), d2 (m, k) float32 (garbage past found)
    -> colours (m, 3) float32."""
    colors = np.ascontiguousarray(np.asarray(colors, f32).reshape(-1, 3))
    m = len(idx)
    h2 = np.where(found == k, d2[:, k - 1], PC.radius_d2_bound(f32(max_distance))).astype(f32)
    blendable = h2 > 0
    C64 = colors.astype(f64)
    S, W = np.zeros((m, 3)), np.zeros(m)
    with np.errstate(all="ignore"):
        for j in range(k):
            use = (j < found) & blendable
            c = C64[np.maximum(idx[:, j], 0)]
            t = d2[:, j].astype(f64) / h2.astype(f64)
            u = 1.0 - t
            w = u * u
            W = W + np.where(use, w, 0.0)
            S = S + np.where(use[:, None], w[:, None] * c, 0.0)
        mean = (S / np.where(W > 0.0, W, 1.0)[:, None]).astype(f32)
    first = colors[np.maximum(idx[:, 0], 0)]
    out = np.where((W > 0.0)[:, None], mean, first)
    return np.where((found > 0)[:, None], out, f32(0)).astype(f32)


def sample_colors(static, colors, queries, k=8, max_distance=np.inf):
    """sdfk_points_blend_colors -> (colours (m, 3) float32, found (m,) int32)."""
    assert 1 <= int(k) <= 64 and f32(max_distance) >= 0
    P = np.ascontiguousarray(np.asarray(static, f32).reshape(-1, 3))
    Q = np.ascontiguousarray(np.asarray(queries, f32).reshape(-1, 3))
    col = _colors(colors, len(P))
    idx, _, found = KM.knn(P, Q, int(k), max_distance)
    with np.errstate(all="ignore"):
        d2 = PC._d2(P, Q, idx)
    return blend_rows(col, d2, found, int(k), max_distance, idx), found.astype(np.int32)


def to_volume(static, normals3, colors, mn, mx, shape, k=8, max_distance=np.inf):
    """sdfk_points_to_volume_colors -> (values (nx, ny, nz) float32, known (nx, ny, nz) bool, colours (nx, ny, nz, 3) float32,
    found (nx, ny, nz) int32): the values of tests/pointcloud_model.to_volume, the colours of sample_colors at the cell centres."""
    assert 1 <= int(k) <= 64 and f32(max_distance) > 0
    P = np.ascontiguousarray(np.asarray(static, f32).reshape(-1, 3))
    N = np.ascontiguousarray(np.asarray(normals3, f32).reshape(-1, 3))
    col = _colors(colors, len(P))
    shape = tuple(int(s) for s in shape)
    Q = PC.centres(mn, mx, shape)
    idx, _, found = KM.knn(P, Q, int(k), max_distance)           # one search feeds both blends, as in the kernel
    value, known = PC.blend(P, N, Q, idx, found, int(k), max_distance)
    sgn = np.where(known, np.where(value < 0, -1, 1), 0).astype(np.int8).reshape(shape)
    far = np.where(PC.fill_signs(sgn) < 0, -f32(max_distance), f32(max_distance)).astype(f32)
    values = np.where(known.reshape(shape), value.reshape(shape), far).astype(f32)
    with np.errstate(all="ignore"):
        d2 = PC._d2(P, Q, idx)
    rgb = blend_rows(col, d2, found, int(k), max_distance, idx)
    return values, known.reshape(shape), rgb.reshape(shape + (3,)), found.reshape(shape).astype(np.int32)


def group_means(colors, group, m):
    """Per channel the mean of every group's members by the rule of the centroid: chunks of 32 members in ascending index, each
    summed in order from +0.0, the chunk sums added in order, (float)(sum / (double)count).  group (n,): the output index of every
    point -> (m, 3) float32."""
    col = np.ascontiguousarray(np.asarray(colors, f32).reshape(-1, 3))
    group = np.asarray(group, np.int64)
    n = len(col)
    order = np.lexsort((np.arange(n), group))                     # by group, members in ascending index
    seg = group[order]
    start = np.flatnonzero(np.concatenate([[True], seg[1:] != seg[:-1]]))
    assert len(start) == m and np.array_equal(seg[start], np.arange(m))
    rank = np.arange(n) - start[seg]
    total, counts = FM.chunked_sums(col[order].astype(f64), seg, rank, m)
    with np.errstate(all="ignore"):
        return (total / counts[:, None].astype(f64)).astype(f32)


def voxel_downsample(static, colors, size, origin=(0, 0, 0)):
    """sdfk_points_voxel_downsample_colors -> (points, counts, group, colours (m, 3) float32)."""
    pts, cnt, group = FM.voxel_downsample(static, size, origin)
    return pts, cnt, group, group_means(_colors(colors, len(group)), group, len(pts))


def end_to_end(fig):
    """The coloured pipeline on the CPU at the grid of tests/golden/pointcloud_accuracy.json (`fig`): the oracle's mesh of a unit
    sphere -> its vertices and normals as a cloud, colours 0.5 + 0.25 p per channel -> the model's coloured, banded volume -> the
    oracle's mesh of that volume.  -> dict: points, normals, colors (the cloud), values, volume_colors (the model's volume), mesh
    (an OracleMesh), color_error = max |mesh.colors - (0.5 + 0.25 mesh.vertices)| in float64.  The colour is an affine function of
    position and a blend reproduces such a function up to the spread of its neighbourhood, so the error measures that spread."""
    from oracle import oracle as O
    n = int(fig["grid"])
    mn, mx = [-1.5] * 3, [1.5] * 3
    scene = O.Scene()
    scene.sphere_w(1.0)
    ov, oc = O.sample(scene, mn, mx, n, n, n)
    first = O.march(ov, oc, mn, mx)
    V = np.ascontiguousarray(first.vertices, f32)
    Nn = np.ascontiguousarray(first.normals, f32)
    col = (f32(0.5) + f32(0.25) * V).astype(f32)
    band = f32(fig["band_voxels"] * (3.0 / n))
    values, _, vcol, _ = to_volume(V, Nn, col, mn, mx, (n, n, n), fig["k"], band)
    mesh = O.march(values, vcol, mn, mx)
    err = float(np.abs(mesh.colors.astype(f64) - (0.5 + 0.25 * mesh.vertices.astype(f64))).max())
    return {"points": V, "normals": Nn, "colors": col, "band": band, "values": values, "volume_colors": vcol, "mesh": mesh,
            "color_error": err}


def accuracy_figures():
    """What tests/golden/pointcloud_color_accuracy.json records (tools/gen_pointcloud_color_accuracy.py writes it)."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "pointcloud_accuracy.json")) as f:
        fig = json.load(f)
    e = end_to_end(fig)
    return {"grid": fig["grid"], "k": fig["k"], "band_voxels": fig["band_voxels"], "cloud_points": int(len(e["points"])),
            "mesh_vertices": int(len(e["mesh"].vertices)), "color": "0.5 + 0.25 p", "vertex_color_error_max": e["color_error"]}
