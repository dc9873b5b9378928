"""Host-side mirror of SdfKit's KdTree (KdTree.cs) and IterativeClosestPoint (IterativeClosestPoint.cs) over the C ABI
entry points sdfk_points_* / sdfk_icp_* (include/sdfkit_hip.h, csrc/lib_points.hip).

Vector3 is a float32 numpy array of 3; a span of Vector3 is an (n, 3) float32 array.  The search is exact (the static
point of least d2, ties to the lowest insertion index; SearchKNearest and
SearchRadius extend it to the k nearest and to all within a radius, in the same (d2, index) order; EstimateNormals, OrientNormals
and ToVoxels turn the points into normals, orient them consistently and make a signed distance volume; VoxelDownsample and
RemoveStatisticalOutliers thin merged scans and drop stray points; Clusters, SelectClusters, RemoveSmallClusters and
LargestCluster tell which points belong together; SampleColors, ToVoxels(colors=) and VoxelDownsample(colors=)
carry per-point colours along); the structure behind it is a grid of cell lists on the device,
so the reference's tree internals -- Left, Right, SplitValue, IsLeaf -- are not provided.  SplitAxis is kept as given.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .raymarch import Matrix4x4

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def _points(points):
    a = np.ascontiguousarray(np.asarray(points, dtype=f32).reshape(-1, 3))
    return a


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else C.c_void_p()


def _per_point(a, n, what):
    """One Vector3 per static point (colours, or anything else averaged like them)."""
    a = _points(a)
    if len(a) != n:
        raise ValueError(f"one {what} per static point ({what}s)")
    return a


class KdTree:
    """KdTree(points, axis=0): the static points, numbered in insertion order."""

    def __init__(self, points, axis=0):
        N.init()
        pts = _points(points)
        h = C.c_void_p()
        N.check(N.lib().sdfk_points_create(_ptr(pts), len(pts), C.byref(h)))
        self._h = h
        self.SplitAxis = int(axis)
        self.Point = pts[0].copy()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and h.value and N._lib is not None and N._inited_device is not None:
            N._lib.sdfk_points_free(h)
        self._h = None

    @property
    def handle(self):
        """The sdfk_points* (extension: for the C ABI's device entry points)."""
        return self._h

    @property
    def TotalPoints(self):
        n = C.c_int64()
        N.check(N.lib().sdfk_points_count(self._h, C.byref(n)))
        return int(n.value)

    def AddPoints(self, points):
        pts = _points(points)
        N.check(N.lib().sdfk_points_add(self._h, _ptr(pts), len(pts)))

    def SearchMany(self, queries):
        """Extension: every query at once -> (indices int32 (-1: none), distances float32, nearest (n, 3) float32)."""
        q = _points(queries)
        n = len(q)
        idx = np.empty(n, np.int32)
        dist = np.empty(n, f32)
        near = np.empty((n, 3), f32)
        if n:
            N.check(N.lib().sdfk_points_search(self._h, _ptr(q), n, _ptr(idx), _ptr(dist), _ptr(near)))
        return idx, dist, near

    def SearchKNearest(self, queries, k, maxDistance=np.inf):
        """Extension: the k nearest static points of every query, ascending by (d2, index), no farther than maxDistance
        -> (indices (n, k) int32, distances (n, k) float32, found (n,) int32); unused slots hold -1 and FLT_MAX.  1 <= k <= 64."""
        q = _points(queries)
        n, k = len(q), int(k)
        if k < 1:   # (no array has such a shape: the library's refusal, without the call)
            raise N.SdfKitNativeError(N.ERR_INVALID, f"sdfk_points_knn: k = {k} is outside [1, 64]")
        idx = np.empty((n, k), np.int32)
        dist = np.empty((n, k), f32)
        found = np.empty(n, np.int32)
        # (n == 0 still goes to the library: it is what refuses a bad k or maxDistance)
        N.check(N.lib().sdfk_points_knn(self._h, _ptr(q), n, k, float(f32(maxDistance)), _ptr(idx), _ptr(dist), _ptr(found)))
        return idx, dist, found

    def SearchRadius(self, queries, radius):
        """Extension: every static point within `radius` of every query (sqrtf(d2) <= radius), as a CSR
        -> (offsets (n + 1,) int64, indices int32, distances float32): query i's neighbours are [offsets[i], offsets[i + 1]),
        ascending by (d2, index)."""
        q = _points(queries)
        n = len(q)
        r = float(f32(radius))
        off = np.zeros(n + 1, np.int64)
        N.check(N.lib().sdfk_points_radius_count(self._h, _ptr(q), n, r, _ptr(off)))
        total = int(off[n])
        idx = np.empty(total, np.int32)
        dist = np.empty(total, f32)
        if total:
            N.check(N.lib().sdfk_points_radius_fill(self._h, _ptr(q), n, r, _ptr(off), _ptr(idx), _ptr(dist)))
        return off, idx, dist

    def SampleColors(self, queries, colors, k=8, maxDistance=np.inf):
        """Extension: the colour at every query from `colors` (one Vector3 per static point): the blend of the k nearest points'
        colours within maxDistance, weighted as ToVoxels weights their distances (k = 1: the nearest point's colour)
        -> (colors (n, 3) float32, found (n,) int32); a query with no point within maxDistance gets (0, 0, 0) and found 0
        (include/sdfkit_hip.h, "Point clouds: colours").  It re-colours the vertices of any mesh from a scan.  Nothing is specific
        to RGB and nothing is clamped: normals can be averaged the same way.  1 <= k <= 64."""
        q = _points(queries)
        col = _per_point(colors, self.TotalPoints, "colour")
        n = len(q)
        out = np.empty((n, 3), f32)
        found = np.empty(n, np.int32)
        # (n == 0 still goes to the library: it is what refuses a bad k or maxDistance)
        N.check(N.lib().sdfk_points_blend_colors(self._h, _ptr(col), _ptr(q), n, int(k), float(f32(maxDistance)), _ptr(out), _ptr(found)))
        return out, found

    def EstimateNormals(self, k, viewpoint=None, maxDistance=np.inf):
        """Extension: a normal per static point from its k nearest (itself included; 3 <= k <= 64, no farther than maxDistance)
        -> (normals (n, 3) float32, variation (n,) float32): the eigenvector of the least eigenvalue of the neighbourhood's
        covariance and the surface variation max(lmin, 0) / (l0 + l1 + l2), never negative and exactly +0 where rounding leaves lmin
        below zero, as on an exact plane (include/sdfkit_hip.h, "Point clouds").  A point with fewer
        than 3 neighbours, or all of them equal, gets (0, 0, 0) and 0.
        viewpoint: one Vector3, or one per point -- each normal is turned towards it.  Without one the component of largest
        magnitude is made positive, which is NOT a consistent orientation of a closed surface: OrientNormals makes one of these
        normals afterwards."""
        n = self.TotalPoints
        view = None if viewpoint is None else _points(viewpoint)
        nrm = np.empty((n, 3), f32)
        var = np.empty(n, f32)
        N.check(N.lib().sdfk_points_normals(self._h, int(k), float(f32(maxDistance)), _ptr(view), 0 if view is None else len(view),
                                            _ptr(nrm), _ptr(var)))
        return nrm, var

    def OrientNormals(self, normals, k=8, maxDistance=np.inf, maxSeeds=64, stats=None):
        """Extension: `normals` (one per static point) with the sign of some flipped, so that neighbouring normals agree and the top
        of every connected piece points up -> (n, 3) float32, bit-identical to the input up to sign (the input is not modified).
        A deterministic region growing over the k-nearest graph (2 <= k <= 64, no farther than maxDistance), confident edges first,
        from at most maxSeeds seeds (include/sdfkit_hip.h, "Point clouds: a consistent orientation").  Normals that are not finite
        or all zero are left alone, and so are those no seed reached.  It trusts that the k nearest of a point lie on the same
        sheet of the surface.  stats: a dict that receives rounds, seeds, flipped, unreached, invalid, levels (a list of 4)."""
        nrm = _points(normals).copy()
        if len(nrm) != self.TotalPoints:
            raise ValueError("one normal per static point (normals)")
        st = (C.c_int64 * 9)()
        N.check(N.lib().sdfk_points_orient_normals(self._h, int(k), float(f32(maxDistance)), int(maxSeeds), _ptr(nrm), st))
        if stats is not None:
            stats.update(rounds=int(st[0]), seeds=int(st[1]), flipped=int(st[2]), unreached=int(st[3]), invalid=int(st[4]),
                         levels=[int(v) for v in st[5:9]])
        return nrm

    def VoxelDownsample(self, voxelSize, origin=(0, 0, 0), colors=None):
        """Extension: one point per occupied voxel of the lattice of edge voxelSize anchored at origin, the centroid of the voxel's
        members -> (points (m, 3) float32, counts (m,) int32, group (n,) int32): the voxels in the order of their lowest member,
        how many points each holds, and the output index of every static point (for averaging further per-point data).
        colors: one Vector3 per static point (colours, or normals); the result then has a fourth element, (m, 3) float32: the
        members' mean per voxel, summed in the order of the centroid.
        A voxelSize below the spacing of the cloud returns the points as they are.  The tree is not changed: make a new KdTree
        from the result.  Refused: a voxelSize that is not finite and positive, a non-finite origin, a cloud spanning 2^21 voxels
        or more along an axis (include/sdfkit_hip.h, "Point clouds: filters")."""
        n = self.TotalPoints
        o = np.ascontiguousarray(np.asarray(origin, dtype=f32).reshape(3))
        pts = np.empty((n, 3), f32)
        cnt = np.empty(n, np.int32)
        group = np.empty(n, np.int32)
        m = C.c_int64()
        if colors is not None:
            col = _per_point(colors, n, "colour")
            out = np.empty((n, 3), f32)
            N.check(N.lib().sdfk_points_voxel_downsample_colors(self._h, float(f32(voxelSize)), _ptr(o), _ptr(col), _ptr(pts), _ptr(cnt), _ptr(group),
                                                                _ptr(out), C.byref(m)))
            return pts[:m.value].copy(), cnt[:m.value].copy(), group, out[:m.value].copy()
        N.check(N.lib().sdfk_points_voxel_downsample(self._h, float(f32(voxelSize)), _ptr(o), _ptr(pts), _ptr(cnt), _ptr(group), C.byref(m)))
        return pts[:m.value].copy(), cnt[:m.value].copy(), group

    def RemoveStatisticalOutliers(self, k, stdRatio, maxDistance=np.inf, stats=None):
        """Extension: the static points whose mean distance to their k nearest (the point itself not counted; 2 <= k <= 64, no
        farther than maxDistance) is at most mu + stdRatio * sigma, mu and sigma the mean and standard deviation of that mean
        distance over the cloud -> (points (kept, 3) float32, indices (kept,) int32 ascending, meanDistance (n,) float32).  A point
        with no neighbour within maxDistance is isolated: its meanDistance is +inf, it takes no part in mu and sigma and is never
        kept.  Per-point data of the kept points, colours for one, is colors[indices].  The tree is not changed: make a new KdTree
        from the result.  stdRatio must be finite and not negative: 0 keeps what is at most the mean, a large finite one keeps
        everything that is not isolated; an infinite one is refused like a NaN (infinity times a sigma of 0 is no number).
        stats: a dict that receives kept, removed, isolated,
        mu, sigma, threshold (include/sdfkit_hip.h, "Point clouds: filters")."""
        n = self.TotalPoints
        pts = np.empty((n, 3), f32)
        idx = np.empty(n, np.int32)
        mean = np.empty(n, f32)
        kept = C.c_int64()
        st = (C.c_int64 * 6)()
        N.check(N.lib().sdfk_points_outliers(self._h, int(k), float(f32(stdRatio)), float(f32(maxDistance)), _ptr(mean), None, _ptr(idx), _ptr(pts),
                                             C.byref(kept), st))
        if stats is not None:
            mu, sigma, thr = np.array(st[3:6], np.int64).view(np.float64)
            stats.update(kept=int(st[0]), removed=int(st[1]), isolated=int(st[2]), mu=float(mu), sigma=float(sigma), threshold=float(thr))
        return pts[:kept.value].copy(), idx[:kept.value].copy(), mean

    def Clusters(self, radius, minPoints=1, stats=None):
        """Extension: density clustering of the static points (DBSCAN; minPoints = 1: Euclidean cluster extraction)
        -> (labels (n,) int32, sizes (C,) int32, core (n,) bool, counts (n,) int32).  counts: the static points within `radius` of
        each point (sqrtf(d2) <= radius, as SearchRadius; the point itself and its duplicates included); a point is core iff its
        count is at least minPoints; clusters are the connected components of the core points under "within radius", numbered by
        their lowest core member; a point that is not core takes the cluster of the core point within the radius that is first in
        (d2, index) order -- so the result does not depend on any order -- and is noise, label -1, without one; sizes counts core
        and border members (include/sdfkit_hip.h, "Point clouds: clusters").  The tree is not changed.  stats: a dict that receives
        clusters, core, border, noise, rounds, shortcuts."""
        n = self.TotalPoints
        labels = np.empty(n, np.int32)
        sizes = np.empty(n, np.int32)
        core = np.empty(n, np.uint8)
        counts = np.empty(n, np.int32)
        c = C.c_int64()
        st = (C.c_int64 * 6)()
        N.check(N.lib().sdfk_points_cluster(self._h, float(f32(radius)), int(minPoints), _ptr(labels), _ptr(sizes), _ptr(core), _ptr(counts),
                                            C.byref(c), st))
        if stats is not None:
            stats.update(clusters=int(st[0]), core=int(st[1]), border=int(st[2]), noise=int(st[3]), rounds=int(st[4]), shortcuts=int(st[5]))
        return labels, sizes[:c.value].copy(), core.astype(bool), counts

    def SelectClusters(self, labels, keep):
        """Extension: the static points whose cluster is kept -> (points (kept, 3) float32, indices (kept,) int32 ascending).
        labels: one int32 per static point, Clusters' or any other; keep: one flag per cluster; a point is kept iff
        0 <= label < len(keep) and keep[label].  Per-point data of the kept points is data[indices]; make a new KdTree from the
        points."""
        n = self.TotalPoints
        lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32).reshape(-1))
        if len(lab) != n:
            raise ValueError("one label per static point (labels)")
        kp = np.ascontiguousarray(np.asarray(keep).astype(bool).reshape(-1).astype(np.uint8))
        pts = np.empty((n, 3), f32)
        idx = np.empty(n, np.int32)
        kept = C.c_int64()
        N.check(N.lib().sdfk_points_select(self._h, _ptr(lab), _ptr(kp), len(kp), _ptr(idx), _ptr(pts), C.byref(kept)))
        return pts[:kept.value].copy(), idx[:kept.value].copy()

    def RemoveSmallClusters(self, radius, minPoints=1, minSize=2, stats=None):
        """Extension: Clusters, then the points of the clusters of at least minSize members; noise goes
        -> (points, indices, labels (n,) int32: Clusters' labels of all static points)."""
        labels, sizes, _, _ = self.Clusters(radius, minPoints, stats)
        pts, idx = self.SelectClusters(labels, sizes >= int(minSize))
        return pts, idx, labels

    def LargestCluster(self, radius, minPoints=1):
        """Extension: Clusters, then the points of the cluster of greatest size (ties: the lowest number) -> (points, indices);
        nothing when there is no cluster."""
        labels, sizes, _, _ = self.Clusters(radius, minPoints)
        keep = np.zeros(len(sizes), bool)
        if len(sizes):
            keep[int(np.argmax(sizes))] = True   # (argmax: the first of the greatest)
        return self.SelectClusters(labels, keep)

    def ToVoxels(self, normals, min, max, nx, ny, nz, k=8, maxDistance=np.inf, clipToBounds=False, stats=None, colors=None):
        """Extension: the point cloud with `normals` (one per static point, pointing outside) as a signed distance volume at the
        cell centres of Voxels(min, max, nx, ny, nz): a blend of the tangent-plane distances (x - p) . n of the k nearest points
        within maxDistance.  Voxels with no point within maxDistance get +-maxDistance, the sign carried over from the known
        ones -- right when the band of known voxels covers a closed surface.  Give a band of a few voxels and call
        Voxels.Redistance() on the result for a full field.  stats: a dict that receives known, unknown, candidates, queries.
        colors: one Vector3 per static point; the volume's Colors are then the same blend of the neighbours' colours (SampleColors
        at every cell centre; zero where no point lies within maxDistance), which Redistance copies and ToMesh interpolates."""
        from .api import Voxels
        vox = Voxels(min, max, nx, ny, nz)
        self.SampleInto(vox, normals, k, maxDistance, stats, colors)
        if clipToBounds:
            vox.ClipToBounds()
        return vox

    def SampleInto(self, voxels, normals, k=8, maxDistance=np.inf, stats=None, colors=None):
        """ToVoxels into an existing Voxels.  Without colors its colours are left alone; with them (one per static point) they are
        overwritten, and a volume made without colour storage gets it."""
        nrm = _points(normals)
        if len(nrm) != self.TotalPoints:
            raise ValueError("one normal per static point (normals)")
        col = None if colors is None else _per_point(colors, self.TotalPoints, "colour")
        if col is not None:
            voxels._ensure_device(True)   # (a device copy without colour storage is dropped: every voxel of it is written below)
        # values the host may have edited go up first: the call writes the distances only, the colours stay what they were
        h = voxels._sync_to_device() if voxels._host_values is not None else voxels._ensure_device(voxels._has_colors)
        st = (C.c_int64 * 4)() if stats is not None else None
        if col is not None:
            N.check(N.lib().sdfk_points_to_volume_colors(self._h, _ptr(nrm), _ptr(col), h, int(k), float(f32(maxDistance)), st))
        else:
            N.check(N.lib().sdfk_points_to_volume(self._h, _ptr(nrm), h, int(k), float(f32(maxDistance)), st))
        voxels._host_values = voxels._host_colors = None   # the device copy is now the truth
        voxels._version += 1
        if stats is not None:
            stats.update(known=int(st[0]), unknown=int(st[1]), candidates=int(st[2]), queries=int(st[3]))
        return voxels

    def Search(self, q):
        """KdTree.Search(q, out nearestDistance) -> (nearest, nearestDistance)."""
        _, d, p = self.SearchMany(np.asarray(q, f32).reshape(1, 3))
        return p[0], f32(d[0])

    def stats(self):
        """sdfk_points_stats: {'grid': (nx, ny, nz), 'candidates', 'queries'} (candidates: last query call under profiling)."""
        s = (C.c_int64 * 5)()
        N.check(N.lib().sdfk_points_stats(self._h, s))
        return {"grid": (s[0], s[1], s[2]), "candidates": int(s[3]), "queries": int(s[4])}


def _is_one_cloud(x):
    if isinstance(x, np.ndarray):
        return x.ndim == 2 or (x.ndim == 1 and x.size == 3)
    try:
        a = np.asarray(x, dtype=f32)
    except ValueError:   # ragged: several clouds
        return False
    return a.ndim == 2 and a.shape[-1] == 3 and not (len(x) and isinstance(x[0], np.ndarray) and x[0].ndim == 2)


class IterativeClosestPoint:
    """IterativeClosestPoint(staticPoints) -- one cloud, or a list of clouds (the ReadOnlyMemory<Vector3>[] overload)."""

    def __init__(self, staticPoints):
        self.MaxIterations = 100
        self.GoodCorrespondenceDistance = f32(0.01)
        self.ConvergedMaximumTranslation = f32(1.0e-4)
        self.ConvergedMaximumRotation = f32(1.0e-5)
        self.Iterations = 0   # extension: iterations of the last RegisterPoints
        self.LastStats = None  # extension: the point-to-plane stats of the last RegisterPoints (None after a point-to-point one)
        self._normals = None
        if _is_one_cloud(staticPoints):
            self._tree = KdTree(staticPoints)
        else:
            clouds = list(staticPoints)
            if not clouds:
                raise ValueError("At least one set of points must be given (staticPoints)")
            self._tree = KdTree(clouds[0])
            for c in clouds[1:]:
                self._tree.AddPoints(c)

    @property
    def StaticTree(self):
        return self._tree

    @property
    def StaticNormals(self):
        """Extension: one normal per static point ((TotalPoints, 3) float32, e.g. StaticTree.EstimateNormals(k)[0]), or None.  With
        normals set, RegisterPoints minimises the distances to the tangent planes at the nearest static points (point to plane);
        their orientation does not matter, and a point whose normal is (0, 0, 0) takes no part."""
        return self._normals

    @StaticNormals.setter
    def StaticNormals(self, normals):
        if normals is None:
            self._normals = None
            return
        a = np.ascontiguousarray(np.asarray(normals, dtype=f32))
        if a.shape != (self._tree.TotalPoints, 3):
            raise ValueError(f"one normal per static point: shape {(self._tree.TotalPoints, 3)} expected, got {a.shape} (StaticNormals)")
        self._normals = a.copy()

    def AddStaticPoints(self, staticPoints, normals=None):
        """normals (extension): the new points' normals -- required when StaticNormals is set, refused when it is not."""
        pts = _points(staticPoints)
        if (normals is None) != (self._normals is None):
            raise ValueError("AddStaticPoints would leave StaticNormals out of step with the static points: "
                             + ("pass normals= for the new points" if normals is None else "set StaticNormals first"))
        if normals is not None:
            nrm = np.ascontiguousarray(np.asarray(normals, dtype=f32))
            if nrm.shape != pts.shape:
                raise ValueError(f"one normal per added point: shape {pts.shape} expected, got {nrm.shape} (normals)")
        self._tree.AddPoints(pts)
        if normals is not None:
            self._normals = np.concatenate([self._normals, nrm])

    def _metric(self, metric):
        if metric is None:
            return "plane" if self._normals is not None else "point"
        if metric not in ("point", "plane"):
            raise ValueError(f"metric must be None, 'point' or 'plane', not {metric!r}")
        if metric == "plane" and self._normals is None:
            raise ValueError("metric='plane' needs StaticNormals")
        return metric

    def _stats(self, st):
        self.LastStats = {"kept": int(st[0]), "sum_r2": float(np.array([st[1]], np.int64).view(np.float64)[0]), "converged": bool(st[2]),
                          "retained": int(st[3]), "raw": [int(v) for v in st]}

    def _params(self):
        return N.IcpParams(int(self.MaxIterations), float(f32(self.GoodCorrespondenceDistance)),
                           float(f32(self.ConvergedMaximumTranslation)), float(f32(self.ConvergedMaximumRotation)))

    def RegisterPoints(self, points, metric=None):
        """Moves `points` -- an (n, 3) float32 C-contiguous array -- in place onto the static points and returns the 4x4 float32
        transform that did it (row-vector convention).  metric (extension): "point" (the reference's step), "plane" (needs
        StaticNormals), or None: "plane" iff StaticNormals is set.  A plane registration leaves its stats in LastStats."""
        metric = self._metric(metric)
        if not (isinstance(points, np.ndarray) and points.dtype == f32 and points.ndim == 2 and points.shape[1] == 3
                and points.flags.c_contiguous and points.flags.writeable):
            raise TypeError("RegisterPoints moves the points in place: pass a writable C-contiguous (n, 3) float32 array")
        prm = self._params()
        total = (C.c_float * 16)()
        iters = C.c_int32()
        if metric == "plane":
            self._check_normals()
            st = (C.c_int64 * 4)()
            N.check(N.lib().sdfk_icp_register_plane(self._tree.handle, C.byref(prm), _ptr(self._normals), _ptr(points), len(points), total,
                                                     C.byref(iters), st))
            self._stats(st)
        else:
            N.check(N.lib().sdfk_icp_register(self._tree.handle, C.byref(prm), _ptr(points), len(points), total, C.byref(iters)))
            self.LastStats = None
        self.Iterations = int(iters.value)
        return np.array(total[:], f32).reshape(4, 4)

    def _check_normals(self):
        if len(self._normals) != self._tree.TotalPoints:   # (points added through StaticTree behind our back)
            raise ValueError("StaticNormals is out of step with the static points")

    def RegisterDevicePoints(self, points_dev, n, metric=None, normals_dev=None):
        """Extension: RegisterPoints on n points (x, y, z float32) already in device memory (a raw pointer), moved in place.
        normals_dev: StaticNormals already in device memory (a raw pointer); without it a plane registration uploads them."""
        metric = self._metric(metric)
        prm = self._params()
        total = (C.c_float * 16)()
        iters = C.c_int32()
        if metric == "plane":
            self._check_normals()
            keep = None
            if normals_dev is None:
                import torch
                keep = torch.from_numpy(self._normals).to(torch.device("cuda", N._inited_device or 0))
                torch.cuda.synchronize()
                normals_dev = keep.data_ptr()
            st = (C.c_int64 * 4)()
            N.check(N.lib().sdfk_icp_register_plane_device(self._tree.handle, C.byref(prm), C.c_void_p(normals_dev), C.c_void_p(points_dev), int(n),
                                                            total, C.byref(iters), st))
            self._stats(st)
            del keep
        else:
            N.check(N.lib().sdfk_icp_register_device(self._tree.handle, C.byref(prm), C.c_void_p(points_dev), int(n), total,
                                                      C.byref(iters)))
            self.LastStats = None
        self.Iterations = int(iters.value)
        return np.array(total[:], f32).reshape(4, 4)

    def GlobalRegisterPoints(self, *args):
        """GlobalRegisterPoints(staticPoints, dynamicPoints) / GlobalRegisterPoints(points) (IterativeClosestPoint.cs:207-240).
        The two-argument form registers against a NEW instance made from staticPoints, as the reference does; each registered
        cloud then joins its static set."""
        if len(args) == 1:
            pts = list(args[0])
            if not pts:
                return []
            if len(pts) == 1:
                return [Matrix4x4.Identity.copy()]
            return self.GlobalRegisterPoints(pts[:1], pts[1:])
        staticPoints, dynamicPoints = args
        dyn = list(dynamicPoints)
        if not dyn:
            return []
        icp = IterativeClosestPoint(list(staticPoints))
        out = []
        for d in dyn:
            out.append(icp.RegisterPoints(d))   # (point to point, as the reference: the new instance has no normals)
            icp.AddStaticPoints(d)
        return out
