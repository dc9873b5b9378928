"""Triangle meshes as signed distance fields over the C ABI entry points sdfk_trimesh_* (include/sdfkit_hip.h,
csrc/lib_trimesh.hip): the exact closest triangle of arbitrary points, signed distance volumes (Mesh -> Voxels), and points
sampled on the triangles in proportion to area (Mesh -> points), and the connectivity of the mesh by index (components, the edge
census, sub-meshes of components: csrc/lib_trimesh_topology.hip), and smoothing and vertex normals over its adjacency
(csrc/lib_trimesh_smooth.hip), and welding: the vertices of equal position made one (csrc/lib_trimesh_weld.hip), and ray casting:
the first hit or any hit of arbitrary rays, and camera renders of the mesh (csrc/lib_trimesh_ray.hip), and the generalized winding
number: is this point inside, for meshes that are open or overlap themselves as well (csrc/lib_trimesh_winding.hip).

The distance is exact (binary64 closest point, ties to the lowest triangle index); the sign is the parity of the mesh's
crossings along z, meaningful for closed meshes (nested shells included) and deterministic for any mesh -- or, with
sign="winding", |winding number| > 1/2, which degrades gracefully on holes and takes the union of overlapping pieces.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _native as N

f32 = np.float32

SAMPLE_STRATIFIED = 1   # SDFK_TRIMESH_SAMPLE_STRATIFIED
SMOOTH_PIN_BOUNDARY = 1  # SDFK_TRIMESH_SMOOTH_PIN_BOUNDARY
NORMALS_FLIP = 1         # SDFK_TRIMESH_NORMALS_FLIP
WELD_KEEP_DEGENERATE = 1    # SDFK_WELD_KEEP_DEGENERATE
WELD_KEEP_UNREFERENCED = 2  # SDFK_WELD_KEEP_UNREFERENCED
SIMPLIFY_PLACEMENTS = {"representative": 0, "centroid": 1, "quadric": 2}   # SDFK_SIMPLIFY_REPRESENTATIVE / _CENTROID / _QUADRIC
SIMPLIFY_DUPLICATES = {"one": 0, "keep": 1, "cancel": 2}                  # 0, SDFK_SIMPLIFY_KEEP_DUPLICATES, SDFK_SIMPLIFY_CANCEL_PAIRS
RAY_ANY_HIT = 1          # SDFK_RAY_ANY_HIT
SIGN_MODES = {"parity": 0, "winding": 1}   # SDFK_TRIMESH_SIGN_PARITY / _WINDING
# The acceptance parameter of the winding number's cluster terms: the smallest beta of the recorded list at which every case of
# tests/golden/mesh_winding_accuracy.json keeps every sign (at 2.0 eight voxels beside the cap of the capped-off sphere flip; at
# 2.5 the worst error of w over the recorded volumes is 2.0e-2, against the threshold's 0.5).
DEFAULT_WINDING_BETA = 2.5

# MeshSdf.SamplePoints: Points (n, 3) f32, Normals (n, 3) f32 (unit face normals), Colors (n, 3) f32 or None, Triangles (n,) int32,
# Weights (n, 3) f32 (the barycentric weights of the triangle's three vertices, as the colour blend used them)
MeshSamples = namedtuple("MeshSamples", "Points Normals Colors Triangles Weights")


class _Rows:
    """The derived quantities of topology rows (one per component, or the census as one row)."""

    @property
    def EulerCharacteristic(self):
        return self.Vertices - self.Edges + self.Triangles

    @property
    def IsWatertight(self):
        """Every edge is used an even number of times: the condition under which ToVoxels' parity sign is well defined."""
        return self.OddEdges == 0

    @property
    def IsOriented(self):
        return (self.InconsistentEdges == 0) & (self.NonManifoldEdges == 0)


class MeshComponents(_Rows):
    """MeshSdf.Components(): Count; VertexLabels (nv,) / TriangleLabels (nt,) int32 (-1: an unreferenced vertex, an
    index-degenerate triangle); per component, as int64 arrays of Count: Triangles, Vertices, Edges, BoundaryEdges,
    NonManifoldEdges, OddEdges, InconsistentEdges, AreaWeights (the sum of the integer sampling weights of the component's
    triangles); and EulerCharacteristic, IsWatertight, IsOriented per component.  Rounds / ShortcutLaunches: what the labels took."""

    def __init__(self, vlabels, tlabels, rows, stats):
        self.Count = len(rows)
        self.VertexLabels, self.TriangleLabels, self.Rows = vlabels, tlabels, rows
        (self.Triangles, self.Vertices, self.Edges, self.BoundaryEdges, self.NonManifoldEdges, self.OddEdges, self.InconsistentEdges,
         self.AreaWeights) = (np.ascontiguousarray(rows[:, k]) for k in range(8))
        self.Rounds, self.ShortcutLaunches = int(stats[0]), int(stats[1])


class MeshTopology(_Rows):
    """MeshSdf.Topology(): the census of the whole mesh as Python ints: Components, Triangles (those that are not
    index-degenerate), Vertices (referenced), Edges, BoundaryEdges, NonManifoldEdges, OddEdges, InconsistentEdges,
    DegenerateTriangles; EulerCharacteristic, IsWatertight, IsOriented as for a component."""

    def __init__(self, census, nt):
        c = [int(x) for x in census]
        self.Census = c
        self.Components, self.Vertices, self.Edges, self.BoundaryEdges, self.NonManifoldEdges, self.OddEdges, self.InconsistentEdges, \
            self.DegenerateTriangles = c
        self.Triangles = int(nt) - self.DegenerateTriangles


# MeshSdf.Select: the kept vertices' old indices, the kept triangles' old indices, the new index array (flat), positions, colours
MeshSelection = namedtuple("MeshSelection", "VertexIndex TriangleIndex Triangles Vertices Colors")


class MeshAdjacency:
    """MeshSdf.Adjacency(): Start (nv + 1,) uint32 and Neighbors uint32 in compressed sparse rows (the neighbours of v are
    Neighbors[Start[v]:Start[v + 1]], ascending, each once); Boundary (nv,) uint8, 1 for the endpoints of an edge with one
    triangle side; Degree (nv,) int64."""

    def __init__(self, start, neighbors, boundary):
        self.Start, self.Neighbors, self.Boundary = start, neighbors, boundary
        self.Degree = np.diff(start.astype(np.int64))

    def Of(self, v):
        return self.Neighbors[self.Start[v]:self.Start[v + 1]]


class MeshWeld:
    """MeshSdf.Weld(): VertexMap (nv,) int32 (the new index of every old vertex's representative, -1: dropped); VertexIndex /
    TriangleIndex int32 (the old index of every new vertex / kept triangle); Vertices, Colors (n, 3) float32 (the representatives'
    own bits; colours zeros when the mesh has none); Triangles int32 (flat, renumbered); Merged (vertices merged away),
    DegenerateDropped, UnreferencedDropped, Passes (radix passes run)."""

    def __init__(self, vmap, vi, ti, tr, vs, cs, stats):
        self.VertexMap, self.VertexIndex, self.TriangleIndex, self.Triangles, self.Vertices, self.Colors = vmap, vi, ti, tr, vs, cs
        self.Merged, self.DegenerateDropped, self.UnreferencedDropped, self.Passes = (int(x) for x in stats)


class MeshSimplify:
    """MeshSdf.Simplify(): MeshWeld's fields -- VertexMap (nv,) int32 (the new number of every old vertex's group, -1: dropped);
    VertexIndex (the representative's old index of every new vertex) / TriangleIndex int32; Vertices, Colors (n, 3) float32 (the
    MADE vertices); Triangles int32 (flat, renumbered); Merged, DegenerateDropped, UnreferencedDropped, Passes -- and
    DuplicatesDropped (triangles dropped for sharing a vertex set with another), QuadricFallbacks (kept groups placed at their
    centroid because the quadric's minimiser did not exist or left the cell)."""

    def __init__(self, vmap, vi, ti, tr, vs, cs, stats):
        self.VertexMap, self.VertexIndex, self.TriangleIndex, self.Triangles, self.Vertices, self.Colors = vmap, vi, ti, tr, vs, cs
        (self.Merged, self.DegenerateDropped, self.DuplicatesDropped, self.UnreferencedDropped, self.Passes,
         self.QuadricFallbacks) = (int(x) for x in stats)


class MeshRayHits:
    """MeshSdf.RayCast(): Triangles (n,) int32 (-1: a miss), Distances (n,) float32 in units of |direction| (+inf: a miss),
    Weights (n, 3) float32 (the barycentric weights of the triangle's three vertices, in SamplePoints' layout; NaN: a miss), Hit
    (n,) bool; Points() -> the hit points origin + direction * distance of the hits, (Hit.sum(), 3) float32, made on the host."""

    def __init__(self, origins, directions, triangles, distances, weights):
        self.Origins, self.Directions = origins, directions
        self.Triangles, self.Distances, self.Weights = triangles, distances, weights
        self.Hit = triangles >= 0

    def Points(self):
        h = self.Hit
        return (self.Origins[h] + self.Directions[h] * self.Distances[h, None]).astype(f32)


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else C.c_void_p()


class MeshSdf:
    """MeshSdf(mesh) or MeshSdf((vertices, triangles[, colors])): the triangles of a Mesh (Vertices, Triangles, Colors) as a
    distance field.  Colours are used only when the mesh has a non-zero colour array."""

    def __init__(self, mesh_or_arrays):
        N.init()
        if isinstance(mesh_or_arrays, (tuple, list)):
            v, t = mesh_or_arrays[0], mesh_or_arrays[1]
            c = mesh_or_arrays[2] if len(mesh_or_arrays) > 2 else None
        else:
            v, t, c = mesh_or_arrays.Vertices, mesh_or_arrays.Triangles, getattr(mesh_or_arrays, "Colors", None)
        self.Vertices = np.ascontiguousarray(np.asarray(v, f32).reshape(-1, 3))
        self.Triangles = np.ascontiguousarray(np.asarray(t, np.int32).reshape(-1))
        cols = None
        if c is not None:
            cols = np.ascontiguousarray(np.asarray(c, f32).reshape(-1, 3))
            if cols.shape != self.Vertices.shape or not np.any(cols):
                cols = None
        self.Colors = cols
        h = C.c_void_p()
        N.check(N.lib().sdfk_trimesh_create(_ptr(self.Vertices), len(self.Vertices), _ptr(self.Triangles), len(self.Triangles),
                                            _ptr(cols) if cols is not None else C.c_void_p(), C.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and h.value and N._lib is not None and N._inited_device is not None:
            N._lib.sdfk_trimesh_free(h)
        self._h = None

    @property
    def handle(self):
        """The sdfk_trimesh* (for the C ABI's device entry points)."""
        return self._h

    def Search(self, points):
        """Every point at once -> (triangle int32 (-1 for a non-finite point), distance float32, closest (n, 3) float32)."""
        q = np.ascontiguousarray(np.asarray(points, f32).reshape(-1, 3))
        n = len(q)
        tri = np.empty(n, np.int32)
        dist = np.empty(n, f32)
        cp = np.empty((n, 3), f32)
        if n:
            N.check(N.lib().sdfk_trimesh_closest(self._h, _ptr(q), n, _ptr(tri), _ptr(dist), _ptr(cp)))
        return tri, dist, cp

    def ToVoxels(self, min, max, nx, ny, nz, maxDistance=float("inf"), clipToBounds=False, sign="parity", beta=DEFAULT_WINDING_BETA):
        """The signed distance at the cell centres of Voxels(min, max, nx, ny, nz) (the centres Voxels.SampleSdf evaluates);
        distances beyond maxDistance become +-maxDistance.  clipToBounds: Voxels.ClipToBounds afterwards.
        sign: "parity" (crossings along z: exact on watertight meshes, streaks on others) or "winding" (|WindingNumber| > 1/2 with
        the acceptance parameter beta: holes are capped by the 1/2 level set and overlapping pieces are united; the values next to
        a cap are distances to the mesh's triangles, not to the cap, until Voxels.Redistance() has run).
        Slow without a band on large volumes far from a fine mesh (every voxel searches until its nearest triangle: the 1.6 M
        triangle sphere into 256^3 takes tens of seconds unbanded, a fraction of a second with a band of a few voxels).  For the far
        field of a large volume, give a band and call Voxels.Redistance() on the result."""
        from .api import Voxels
        vox = Voxels(min, max, nx, ny, nz)
        self.SampleInto(vox, maxDistance, sign, beta)
        if clipToBounds:
            vox.ClipToBounds()
        return vox

    def SampleInto(self, voxels, maxDistance=float("inf"), sign="parity", beta=DEFAULT_WINDING_BETA):
        """Writes the signed distance (and, when the mesh has colours, the blended colours) into an existing Voxels."""
        if sign not in SIGN_MODES:
            raise ValueError(f"sign must be one of {sorted(SIGN_MODES)}")
        h = voxels._ensure_device(self.Colors is not None or voxels._has_colors)
        if sign == "parity":
            N.check(N.lib().sdfk_trimesh_to_volume(self._h, h, C.c_float(maxDistance)))
        else:
            N.check(N.lib().sdfk_trimesh_to_volume_signed(self._h, h, C.c_float(maxDistance), SIGN_MODES[sign], C.c_float(beta)))
        voxels._host_values = voxels._host_colors = None   # the device copy is now the truth
        voxels._version += 1
        return voxels

    def SamplePoints(self, n, seed=0, stratified=True):
        """n points on the triangles, in proportion to area (sdfk_trimesh_sample: one stated function of the mesh, n, seed and
        the mode, the same bits on every run) -> MeshSamples.  Normals are the unit face normals of the winding (b - a) x (c - a),
        which on marching-cubes meshes point the way the vertex normals do; Colors the blended vertex colours (None when the mesh
        has none); any other per-vertex attribute blends as attr[tri[Triangles]] weighted by Weights.  stratified: one sample per
        equal share of the total area (every triangle gets its share to within two samples, and the output follows the triangle
        order); otherwise independent draws, and sample s does not depend on n.  A triangle whose area is below 2^-32 of the largest
        one is never sampled; a mesh in which no triangle has an area is refused."""
        n, seed, flags = int(n), C.c_uint64(int(seed) & (2 ** 64 - 1)), SAMPLE_STRATIFIED if stratified else 0
        if not 0 <= n < 2 ** 31:   # (the library refuses it: nothing is allocated for it first)
            N.check(N.lib().sdfk_trimesh_sample(self._h, n, seed, flags, None, None, None, None, None, None))
        pts, nrm, wts = np.empty((n, 3), f32), np.empty((n, 3), f32), np.empty((n, 3), f32)
        tri = np.empty(n, np.int32)
        cols = np.empty((n, 3), f32) if self.Colors is not None else None
        N.check(N.lib().sdfk_trimesh_sample(self._h, n, seed, flags, _ptr(pts), _ptr(nrm), _ptr(cols) if cols is not None else C.c_void_p(),
                                            _ptr(tri), _ptr(wts), None))
        return MeshSamples(pts, nrm, cols, tri, wts)

    def SamplePointsDevice(self, n, seed, stratified, points_dev, normals_dev=None, colors_dev=None, triangles_dev=None, weights_dev=None):
        """SamplePoints into caller-owned device memory (raw pointers; None: that output is not wanted): after the handle's first
        sampling call this only queues work on the library stream."""
        N.check(N.lib().sdfk_trimesh_sample_device(self._h, int(n), C.c_uint64(int(seed) & (2 ** 64 - 1)), SAMPLE_STRATIFIED if stratified else 0,
                                                   *[C.c_void_p(p) if p else C.c_void_p() for p in (points_dev, normals_dev, colors_dev,
                                                                                                   triangles_dev, weights_dev)], None))

    def sample_stats(self):
        """{"sampled_triangles": triangles of non-zero sampling weight, "total_weight": the sum of the integer weights (the largest
        triangle has 2^32)}; makes the weights when no sampling call has."""
        s = (C.c_int64 * 2)()
        N.check(N.lib().sdfk_trimesh_sample(self._h, 1, C.c_uint64(0), 0, None, None, None, None, None, s))
        return {"sampled_triangles": int(s[0]), "total_weight": int(s[1])}

    def Components(self):
        """The connected components by index (sdfk_trimesh_components, sdfk_trimesh_topology) -> MeshComponents.  Two vertices
        with equal positions and different indices are different vertices."""
        nv, nt = len(self.Vertices), len(self.Triangles) // 3
        vl, tl = np.empty(nv, np.int32), np.empty(nt, np.int32)
        n, st = C.c_int64(), (C.c_int64 * 4)()
        N.check(N.lib().sdfk_trimesh_components(self._h, _ptr(vl), _ptr(tl), C.byref(n), st))
        rows = np.zeros((n.value, 8), np.int64)
        census = (C.c_int64 * 8)()
        N.check(N.lib().sdfk_trimesh_topology(self._h, census, _ptr(rows), n.value))
        return MeshComponents(vl, tl, rows, st)

    def Topology(self):
        """The edge census of the whole mesh (sdfk_trimesh_topology) -> MeshTopology."""
        census = (C.c_int64 * 8)()
        N.check(N.lib().sdfk_trimesh_topology(self._h, census, None, 0))
        return MeshTopology(census[:], len(self.Triangles) // 3)

    def Select(self, keep):
        """The sub-mesh of the components whose flag in `keep` (one per component) is set (sdfk_trimesh_select) ->
        MeshSelection; vertices and triangles keep their order and triangles are renumbered."""
        n = C.c_int64()
        N.check(N.lib().sdfk_trimesh_components(self._h, None, None, C.byref(n), None))
        k = np.ascontiguousarray(np.asarray(keep).astype(bool).reshape(-1).astype(np.uint8))
        if len(k) != n.value:
            raise ValueError(f"keep has {len(k)} flags, the mesh has {n.value} components")
        k = np.append(k, np.uint8(0))   # (never empty: a NULL keep array is refused)
        nv, nt = len(self.Vertices), len(self.Triangles) // 3
        vi, ti, tr = np.empty(nv, np.int32), np.empty(nt, np.int32), np.empty(3 * nt, np.int32)
        vs, cs = np.empty((nv, 3), f32), np.empty((nv, 3), f32)
        kv, kt = C.c_int64(), C.c_int64()
        N.check(N.lib().sdfk_trimesh_select(self._h, _ptr(k), _ptr(vi), _ptr(ti), _ptr(tr), _ptr(vs), _ptr(cs), C.byref(kv), C.byref(kt)))
        kv, kt = kv.value, kt.value
        return MeshSelection(vi[:kv].copy(), ti[:kt].copy(), tr[:3 * kt].copy(), vs[:kv].copy(), cs[:kv].copy())

    def Adjacency(self):
        """The neighbours of every vertex, ascending and each once, and the boundary bytes (sdfk_trimesh_adjacency) ->
        MeshAdjacency.  Made once per handle and kept on it."""
        nv = len(self.Vertices)
        n = C.c_int64()
        N.check(N.lib().sdfk_trimesh_adjacency(self._h, None, None, None, C.byref(n)))
        start, nbr, boundary = np.empty(nv + 1, np.uint32), np.empty(n.value, np.uint32), np.empty(nv, np.uint8)
        N.check(N.lib().sdfk_trimesh_adjacency(self._h, _ptr(start), _ptr(nbr), _ptr(boundary), None))
        return MeshAdjacency(start, nbr, boundary)

    @staticmethod
    def _smooth_flags(pinBoundary):
        return SMOOTH_PIN_BOUNDARY if pinBoundary else 0

    def Smooth(self, iterations, lam=0.5, mu=-0.53, pinBoundary=True):
        """The positions after `iterations` iterations of Taubin's lambda | mu smoothing (sdfk_trimesh_smooth: one stated function
        of the mesh and the arguments) -> (nv, 3) float32.  An iteration is a step with lam, then, if mu != 0, a step with mu; a
        step moves every vertex by the factor towards the mean of its neighbours (by index, each once).  mu = 0: plain Laplacian
        smoothing, which shrinks.  pinBoundary: the vertices of edges with one triangle side stay where they are.  This handle is
        not changed: its distance queries still see the old positions."""
        out = np.empty((len(self.Vertices), 3), f32)
        N.check(N.lib().sdfk_trimesh_smooth(self._h, int(iterations), C.c_float(lam), C.c_float(mu), self._smooth_flags(pinBoundary), _ptr(out)))
        return out

    def SmoothDevice(self, iterations, lam, mu, pinBoundary, vertices_dev):
        """Smooth into caller-owned device memory (a raw pointer to nv x 3 floats): once the handle has its adjacency this only
        queues the steps on the library stream."""
        N.check(N.lib().sdfk_trimesh_smooth_device(self._h, int(iterations), C.c_float(lam), C.c_float(mu), self._smooth_flags(pinBoundary),
                                                   C.c_void_p(vertices_dev) if vertices_dev else C.c_void_p()))

    def VertexNormals(self, positions=None, flip=False):
        """Area-weighted unit vertex normals from the geometry (sdfk_trimesh_vertex_normals) -> (nv, 3) float32: the normalised sum
        of (b - a) x (c - a) over the triangles at each vertex, zeros where there is none.  positions: (nv, 3) to use in place of
        the handle's own (the output of Smooth, say).  On marching-cubes meshes the unflipped normals point the way the gradient
        normals do."""
        nv = len(self.Vertices)
        p = None
        if positions is not None:
            p = np.ascontiguousarray(np.asarray(positions, f32).reshape(-1, 3))
            if len(p) != nv:
                raise ValueError(f"positions has {len(p)} rows, the mesh has {nv} vertices")
        out = np.empty((nv, 3), f32)
        N.check(N.lib().sdfk_trimesh_vertex_normals(self._h, _ptr(p) if p is not None else C.c_void_p(), NORMALS_FLIP if flip else 0, _ptr(out)))
        return out

    def VertexNormalsDevice(self, positions_dev, flip, normals_dev):
        """VertexNormals from and into caller-owned device memory (raw pointers; positions_dev None: the handle's own positions)."""
        N.check(N.lib().sdfk_trimesh_vertex_normals_device(self._h, C.c_void_p(positions_dev) if positions_dev else C.c_void_p(),
                                                           NORMALS_FLIP if flip else 0, C.c_void_p(normals_dev) if normals_dev else C.c_void_p()))

    @staticmethod
    def _weld_flags(keepDegenerate, keepUnreferenced):
        return (WELD_KEEP_DEGENERATE if keepDegenerate else 0) | (WELD_KEEP_UNREFERENCED if keepUnreferenced else 0)

    def Weld(self, tolerance=0.0, keepDegenerate=False, keepUnreferenced=False):
        """The mesh with the vertices of equal position made one (sdfk_trimesh_weld: one stated function of the mesh and the
        arguments) -> MeshWeld.  tolerance 0: positions equal as values (-0 equals +0); tolerance > 0: the vertices of one cell
        of the lattice of that size anchored at the origin -- a lattice, not a ball query: two vertices closer than the tolerance
        on opposite sides of a cell face do not weld.  A group is replaced by its lowest index, which keeps its own position and
        colour; triangles that become index-degenerate and representatives no kept triangle names are dropped unless the flags
        keep them.  This handle is not changed."""
        nv, nt = len(self.Vertices), len(self.Triangles) // 3
        vm, vi, ti, tr = np.empty(nv, np.int32), np.empty(nv, np.int32), np.empty(nt, np.int32), np.empty(3 * nt, np.int32)
        vs, cs = np.empty((nv, 3), f32), np.empty((nv, 3), f32)
        kv, kt, st = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
        N.check(N.lib().sdfk_trimesh_weld(self._h, C.c_float(tolerance), self._weld_flags(keepDegenerate, keepUnreferenced), _ptr(vm), _ptr(vi),
                                          _ptr(ti), _ptr(tr), _ptr(vs), _ptr(cs), C.byref(kv), C.byref(kt), st))
        kv, kt = kv.value, kt.value
        return MeshWeld(vm, vi[:kv].copy(), ti[:kt].copy(), tr[:3 * kt].copy(), vs[:kv].copy(), cs[:kv].copy(), st[:])

    def WeldDevice(self, tolerance, keepDegenerate, keepUnreferenced, vertex_map_dev=None, vertex_index_dev=None, triangle_index_dev=None,
                   triangles_dev=None, vertices_dev=None, colors_dev=None):
        """Weld into caller-owned device memory (raw pointers; None: that output is not wanted) -> (vertices, triangles, stats):
        the counts and the four stats.  The outputs are ready for sdfk_trimesh_create_device."""
        kv, kt, st = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
        N.check(N.lib().sdfk_trimesh_weld_device(self._h, C.c_float(tolerance), self._weld_flags(keepDegenerate, keepUnreferenced),
                                                 *[C.c_void_p(p) if p else C.c_void_p() for p in (vertex_map_dev, vertex_index_dev, triangle_index_dev,
                                                                                                 triangles_dev, vertices_dev, colors_dev)],
                                                 C.byref(kv), C.byref(kt), st))
        return kv.value, kt.value, [int(x) for x in st]

    @staticmethod
    def _simplify_codes(placement, duplicates):
        if placement not in SIMPLIFY_PLACEMENTS:
            raise ValueError(f"placement must be one of {sorted(SIMPLIFY_PLACEMENTS)}")
        if duplicates not in SIMPLIFY_DUPLICATES:
            raise ValueError(f"duplicates must be one of {sorted(SIMPLIFY_DUPLICATES)}")
        return SIMPLIFY_PLACEMENTS[placement], SIMPLIFY_DUPLICATES[duplicates]

    def Simplify(self, cellSize, placement="quadric", duplicates="one"):
        """The mesh made smaller by vertex clustering (sdfk_trimesh_simplify: one stated function of the mesh and the arguments)
        -> MeshSimplify.  The vertices of one cell of the lattice of size cellSize anchored at the origin become one vertex:
        placement "representative" (the lowest index, as it is), "centroid" (the mean of the cell's vertices) or "quadric" (the
        point nearest the planes of the cell's triangles, kept inside the cell; the centroid where that fails).  Triangles that
        become index-degenerate are dropped; of those that come to share a vertex set, duplicates "one" keeps the lowest index,
        "keep" all, "cancel" the lowest index of an odd number and none of an even one -- which keeps a watertight mesh
        watertight.  This handle is not changed."""
        code, flags = self._simplify_codes(placement, duplicates)
        nv, nt = len(self.Vertices), len(self.Triangles) // 3
        vm, vi, ti, tr = np.empty(nv, np.int32), np.empty(nv, np.int32), np.empty(nt, np.int32), np.empty(3 * nt, np.int32)
        vs, cs = np.empty((nv, 3), f32), np.empty((nv, 3), f32)
        kv, kt, st = C.c_int64(), C.c_int64(), (C.c_int64 * 6)()
        N.check(N.lib().sdfk_trimesh_simplify(self._h, C.c_float(cellSize), code, flags, _ptr(vm), _ptr(vi), _ptr(ti), _ptr(tr), _ptr(vs),
                                              _ptr(cs), C.byref(kv), C.byref(kt), st))
        kv, kt = kv.value, kt.value
        return MeshSimplify(vm, vi[:kv].copy(), ti[:kt].copy(), tr[:3 * kt].copy(), vs[:kv].copy(), cs[:kv].copy(), st[:])

    def SimplifyDevice(self, cellSize, placement, duplicates, vertex_map_dev=None, vertex_index_dev=None, triangle_index_dev=None,
                       triangles_dev=None, vertices_dev=None, colors_dev=None):
        """Simplify into caller-owned device memory (raw pointers; None: that output is not wanted) -> (vertices, triangles, stats):
        the counts and the six stats.  The outputs are ready for sdfk_trimesh_create_device."""
        code, flags = self._simplify_codes(placement, duplicates)
        kv, kt, st = C.c_int64(), C.c_int64(), (C.c_int64 * 6)()
        N.check(N.lib().sdfk_trimesh_simplify_device(self._h, C.c_float(cellSize), code, flags,
                                                     *[C.c_void_p(p) if p else C.c_void_p() for p in (vertex_map_dev, vertex_index_dev,
                                                                                                     triangle_index_dev, triangles_dev, vertices_dev,
                                                                                                     colors_dev)],
                                                     C.byref(kv), C.byref(kt), st))
        return kv.value, kt.value, [int(x) for x in st]

    @staticmethod
    def _rays(origins, directions):
        o = np.ascontiguousarray(np.asarray(origins, f32).reshape(-1, 3))
        d = np.ascontiguousarray(np.asarray(directions, f32).reshape(-1, 3))
        if len(d) != len(o):
            if len(o) != 1:
                raise ValueError(f"{len(o)} origins for {len(d)} directions")
            o = np.ascontiguousarray(np.broadcast_to(o, d.shape))   # (one origin for every direction)
        return o, d

    def RayCast(self, origins, directions, tMin=0.0, tMax=float("inf")):
        """The first hit of every ray origin + t direction, tMin <= t <= tMax (sdfk_trimesh_raycast: one stated function of the
        mesh, the rays and the range; the watertight ray-triangle test in binary64, ties to the lowest triangle index) ->
        MeshRayHits.  Directions need not be unit vectors: t, and so Distances, is in units of |direction|.  One origin may be
        given for all directions.  A ray with a NaN or infinite component or a zero direction is a miss."""
        o, d = self._rays(origins, directions)
        n = len(o)
        tri, dist, w = np.empty(n, np.int32), np.empty(n, f32), np.empty((n, 3), f32)
        N.check(N.lib().sdfk_trimesh_raycast(self._h, _ptr(o), _ptr(d), n, C.c_float(tMin), C.c_float(tMax), 0, _ptr(tri), _ptr(dist), _ptr(w)))
        return MeshRayHits(o, d, tri, dist, w)

    def RayCastDevice(self, origins_dev, directions_dev, n, tMin=0.0, tMax=float("inf"), triangles_dev=None, distances_dev=None, weights_dev=None,
                      anyHit=False):
        """RayCast from and into caller-owned device memory (raw pointers; None: that output is not wanted): only queues work on
        the library stream.  anyHit: the occlusion query of Occluded (triangles 0 / -1; no distances, no weights)."""
        N.check(N.lib().sdfk_trimesh_raycast_device(self._h, *[C.c_void_p(p) if p else C.c_void_p() for p in (origins_dev, directions_dev)], int(n),
                                                    C.c_float(tMin), C.c_float(tMax), RAY_ANY_HIT if anyHit else 0,
                                                    *[C.c_void_p(p) if p else C.c_void_p() for p in (triangles_dev, distances_dev, weights_dev)]))

    def Occluded(self, origins, directions, tMin=0.0, tMax=float("inf")):
        """Whether anything is hit within the range, per ray (sdfk_trimesh_raycast with SDFK_RAY_ANY_HIT: the search stops at the
        first hit it meets) -> (n,) bool, equal to RayCast(...).Hit.  For the line of sight between a sensor s and a point p:
        Occluded(s, p - s, tMin, 1 - margin)."""
        o, d = self._rays(origins, directions)
        n = len(o)
        tri = np.empty(n, np.int32)
        N.check(N.lib().sdfk_trimesh_raycast(self._h, _ptr(o), _ptr(d), n, C.c_float(tMin), C.c_float(tMax), RAY_ANY_HIT, _ptr(tri), None, None))
        return tri >= 0

    @staticmethod
    def _camera(width, height, camera, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance):
        """RayMarcher's own camera: the position and the inverse view-projection of (viewTransform,) or (position, target, up)"""
        from .raymarch import Matrix4x4, RayMarcher
        rm = RayMarcher(width, height, None)
        if camera:
            rm.ViewTransform = np.asarray(camera[0], f32) if len(camera) == 1 else Matrix4x4.CreateLookAt(*camera)
        if verticalFieldOfViewDegrees is not None:
            rm.VerticalFieldOfViewDegrees = verticalFieldOfViewDegrees
        if nearPlaneDistance is not None:
            rm.NearPlaneDistance = nearPlaneDistance
        if farPlaneDistance is not None:
            rm.FarPlaneDistance = farPlaneDistance
        return rm.camera() + (rm.NearPlaneDistance, rm.FarPlaneDistance)

    def _render(self, width, height, camera, lens, want_depth, want_rgb, want_triangles):
        width, height = int(width), int(height)
        unknown = set(lens) - {"verticalFieldOfViewDegrees", "nearPlaneDistance", "farPlaneDistance"}
        if unknown:
            raise TypeError(f"unknown arguments {sorted(unknown)}")
        if width < 1 or height < 1:   # (the library refuses it; there is no camera of such an image to derive first)
            N.check(N.lib().sdfk_trimesh_render(self._h, width, height, N.f3((0, 0, 0)), (C.c_float * 16)(), C.c_float(0), C.c_float(1), None, None, None))
        pos, vpi, near, far = self._camera(width, height, camera, lens.get("verticalFieldOfViewDegrees"), lens.get("nearPlaneDistance"),
                                           lens.get("farPlaneDistance"))
        shape = (max(height, 0), max(width, 0))
        depth = np.empty(shape, f32) if want_depth else None
        rgb = np.empty(shape + (3,), f32) if want_rgb else None
        tri = np.empty(shape, np.int32) if want_triangles else None
        N.check(N.lib().sdfk_trimesh_render(self._h, width, height, N.f3(pos), (C.c_float * 16)(*[float(x) for x in vpi.ravel()]), C.c_float(near),
                                            C.c_float(far), *[a.ctypes.data if a is not None else None for a in (depth, rgb, tri)]))
        return depth, rgb, tri

    def Render(self, width, height, *camera, **lens):
        """The mesh as one camera sees it, Lambert-shaded with RayMarcher's light and sky (sdfk_trimesh_render) -> Vec3Data.
        camera: nothing (RayMarcher's default view), a view transform, or position, target, up; lens: verticalFieldOfViewDegrees,
        nearPlaneDistance, farPlaneDistance -- RayMarcher's, with its defaults.  Vertex colours are blended; a mesh without is white."""
        from .raymarch import Vec3Data
        return Vec3Data(self._render(width, height, camera, lens, False, True, False)[1])

    def RenderDepth(self, width, height, *camera, **lens):
        """The distance along every pixel's ray to the first surface between the near and the far plane, +inf where there is none
        -> FloatData: a depth image as RayMarcher.RenderDepth makes of an SDF."""
        from .raymarch import FloatData
        return FloatData(self._render(width, height, camera, lens, True, False, False)[0])

    def RenderTriangles(self, width, height, *camera, **lens):
        """The index of the triangle every pixel sees, -1 for the sky -> (height, width) int32."""
        return self._render(width, height, camera, lens, False, False, True)[2]

    def RenderDevice(self, width, height, camera_position, view_projection_inverse, nearPlaneDistance, farPlaneDistance, depth_dev=None, rgb_dev=None,
                     triangles_dev=None):
        """sdfk_trimesh_render_device: the images into caller-owned device memory (raw pointers; None: not wanted), queued on the
        library stream.  camera_position (3) and view_projection_inverse (4 x 4) as RayMarcher.camera() returns them."""
        N.check(N.lib().sdfk_trimesh_render_device(self._h, int(width), int(height), N.f3(camera_position),
                                                   (C.c_float * 16)(*[float(x) for x in np.asarray(view_projection_inverse, f32).ravel()]),
                                                   C.c_float(nearPlaneDistance), C.c_float(farPlaneDistance),
                                                   *[C.c_void_p(p) if p else C.c_void_p() for p in (depth_dev, rgb_dev, triangles_dev)]))

    def _winding(self, points, beta, want_winding, want_inside):
        q = np.ascontiguousarray(np.asarray(points, f32).reshape(-1, 3))
        n = len(q)
        w = np.empty(n, f32) if want_winding else None
        inside = np.empty(n, np.uint8) if want_inside else None
        N.check(N.lib().sdfk_trimesh_winding(self._h, _ptr(q), n, C.c_float(beta), _ptr(w), _ptr(inside)))
        return w, inside

    def WindingNumber(self, points, beta=DEFAULT_WINDING_BETA):
        """The generalized winding number of every point (sdfk_trimesh_winding: one stated function of the mesh, the point and
        beta) -> (n,) float32: on a closed, consistently oriented mesh 0 outside and +1 (outward-facing triangles) or -1 inside, 2
        where closed pieces overlap, 0 in a cavity; a smooth function where the mesh is open; NaN for a point with a NaN or
        infinite coordinate.  Clusters of triangles farther than beta times their radius are replaced by their first-order term;
        beta = inf sums every triangle.  The hierarchy is made by the handle's first call and kept."""
        return self._winding(points, beta, True, False)[0]

    def Contains(self, points, beta=DEFAULT_WINDING_BETA):
        """Whether each point is inside the mesh: |winding number| > 1/2, decided in binary64 before the rounding to float32 ->
        (n,) bool.  Independent of which way the normals point; the union of overlapping closed pieces; holes are capped by the
        1/2 level set."""
        return self._winding(points, beta, False, True)[1].astype(bool)

    def WindingNumberDevice(self, points_dev, n, beta=DEFAULT_WINDING_BETA, winding_dev=None, inside_dev=None):
        """WindingNumber / Contains from and into caller-owned device memory (raw pointers; None: that output is not wanted;
        inside is one byte per point): once the handle has its hierarchy this only queues work on the library stream."""
        N.check(N.lib().sdfk_trimesh_winding_device(self._h, C.c_void_p(points_dev) if points_dev else C.c_void_p(), int(n), C.c_float(beta),
                                                    *[C.c_void_p(p) if p else C.c_void_p() for p in (winding_dev, inside_dev)]))

    def winding_stats(self):
        """sdfk_trimesh_winding_stats: the hierarchy (levels -1 before the first winding call) and the term counts of the last
        profiled call."""
        s = (C.c_int64 * 8)()
        N.check(N.lib().sdfk_trimesh_winding_stats(self._h, s))
        return {"levels": int(s[0]), "occupied_nodes": int(s[1]), "largest_leaf": int(s[2]), "builds": int(s[3]), "cluster_terms": int(s[4]),
                "triangle_terms": int(s[5]), "queries": int(s[6]), "nodes": int(s[7])}

    def stats(self):
        """sdfk_trimesh_stats: grid, triangles, binned pairs, candidates / queries of the last profiled call, crossings."""
        s = (C.c_int64 * 8)()
        N.check(N.lib().sdfk_trimesh_stats(self._h, s))
        return {"grid": (s[0], s[1], s[2]), "triangles": int(s[3]), "entries": int(s[4]), "candidates": int(s[5]),
                "queries": int(s[6]), "crossings": int(s[7])}
