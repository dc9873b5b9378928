// KdTree.Hip.cs -- SdfKit.KdTree over sdfk_points_* (include/sdfkit_hip.h).  Replaces SdfKit/KdTree.cs: the public members
// keep their names and meaning (KdTree.cs:8-198), the search is exact (ties to the lowest insertion index, a documented
// deviation: the reference returns whichever point its traversal met first).  The tree internals -- Left, Right,
// SplitValue, IsLeaf -- have no counterpart: the structure is a grid of cell lists on the GPU.
// UNCOMPILED HERE (no .NET in the build image); sdfkit_amd/points.py's KdTree is the same layer, tested.
using System;
using System.Numerics;
using SdfKit.Hip;

namespace SdfKit
{
    public class KdTree : IDisposable
    {
        IntPtr handle;   // sdfk_points*

        public Vector3 Point;
        /// <summary>0 = x, 1 = y, 2 = z (kept as given; the GPU structure does not split)</summary>
        public readonly byte SplitAxis;

        public KdTree (ReadOnlySpan<Vector3> points, byte axis = 0)
        {
            if (points.Length == 0)
                throw new ArgumentException ("At least on point must be given", nameof (points));
            Native.EnsureInit ();
            Point = points[0];
            SplitAxis = axis;
            unsafe {
                fixed (Vector3* p = points)
                    Native.Check (Native.sdfk_points_create ((float*)p, points.Length, out handle));
            }
        }

        internal IntPtr Handle => handle;

        public int TotalPoints {
            get {
                Native.Check (Native.sdfk_points_count (handle, out var n));
                return (int)n;
            }
        }

        public void AddPoints (ReadOnlySpan<Vector3> points)
        {
            if (points.Length == 0)
                return;
            unsafe {
                fixed (Vector3* p = points)
                    Native.Check (Native.sdfk_points_add (handle, (float*)p, points.Length));
            }
        }

        public unsafe Vector3 Search (Vector3 q, out float nearestDistance)
        {
            Vector3 nearest;
            float d;
            Native.Check (Native.sdfk_points_search (handle, (float*)&q, 1, null, &d, (float*)&nearest));
            nearestDistance = d;
            return nearest;   // (no point counts: Point and float.MaxValue, as the reference)
        }

        /// <summary>Extension: every query at once; index -1 where no point counts.</summary>
        public unsafe void Search (ReadOnlySpan<Vector3> queries, Span<int> indices, Span<float> distances, Span<Vector3> nearest)
        {
            if (indices.Length < queries.Length || distances.Length < queries.Length || nearest.Length < queries.Length)
                throw new ArgumentException ("Output spans are shorter than the queries");
            fixed (Vector3* q = queries) fixed (int* i = indices) fixed (float* d = distances) fixed (Vector3* n = nearest)
                Native.Check (Native.sdfk_points_search (handle, (float*)q, queries.Length, i, d, (float*)n));
        }

        /// <summary>Extension: the k nearest static points of every query (1..64), ascending by (d2, index), no farther than
        /// maxDistance.  indices / distances hold queries.Length rows of k (-1 and float.MaxValue in unused slots), found the
        /// number of real entries per query.</summary>
        public unsafe void SearchKNearest (ReadOnlySpan<Vector3> queries, int k, Span<int> indices, Span<float> distances, Span<int> found,
                                           float maxDistance = float.PositiveInfinity)
        {
            if (k < 1 || k > 64)
                throw new ArgumentOutOfRangeException (nameof (k), "k must be in 1..64 (larger neighbourhoods: SearchRadius)");
            long nk = (long)queries.Length * k;
            if (indices.Length < nk || distances.Length < nk || found.Length < queries.Length)
                throw new ArgumentException ("Output spans are shorter than queries x k");
            fixed (Vector3* q = queries) fixed (int* i = indices) fixed (float* d = distances) fixed (int* f = found)
                Native.Check (Native.sdfk_points_knn (handle, (float*)q, queries.Length, k, maxDistance, i, d, f));
        }

        /// <summary>Extension: every static point within radius of every query (distance &lt;= radius), as a CSR: query i's
        /// neighbours are [offsets[i], offsets[i + 1]), ascending by (d2, index).</summary>
        public unsafe void SearchRadius (ReadOnlySpan<Vector3> queries, float radius, out long[] offsets, out int[] indices, out float[] distances)
        {
            offsets = new long[queries.Length + 1];
            fixed (Vector3* q = queries) fixed (long* o = offsets) {
                Native.Check (Native.sdfk_points_radius_count (handle, (float*)q, queries.Length, radius, o));
                indices = new int[offsets[queries.Length]];
                distances = new float[indices.Length];
                if (indices.Length > 0)
                    fixed (int* i = indices) fixed (float* d = distances)
                        Native.Check (Native.sdfk_points_radius_fill (handle, (float*)q, queries.Length, radius, o, i, d));
            }
        }

        /// <summary>Extension: a normal per static point (insertion order) from its k nearest (3..64, itself included, no farther than
        /// maxDistance): the eigenvector of the least eigenvalue of the neighbourhood's covariance, and the surface variation
        /// max(lmin, 0) / (l0 + l1 + l2), never negative (exactly +0 on an exact plane).  viewpoints: empty (the largest component is made positive -- not a consistent orientation of
        /// a closed surface: OrientNormals makes one afterwards), one for all points, or one per point; each normal is turned towards its
        /// viewpoint.  Degenerate neighbourhoods give (0, 0, 0) and 0.</summary>
        public unsafe void EstimateNormals (int k, Span<Vector3> normals, Span<float> variation, ReadOnlySpan<Vector3> viewpoints = default,
                                            float maxDistance = float.PositiveInfinity)
        {
            if (k < 3 || k > 64)
                throw new ArgumentOutOfRangeException (nameof (k), "k must be in 3..64");
            int n = TotalPoints;
            if (normals.Length < n || variation.Length < n)
                throw new ArgumentException ("Output spans are shorter than the static points");
            fixed (Vector3* v = viewpoints) fixed (Vector3* o = normals) fixed (float* w = variation)
                Native.Check (Native.sdfk_points_normals (handle, k, maxDistance, (float*)v, viewpoints.Length, (float*)o, w));
        }

        /// <summary>Extension: flips the sign of some of `normals` (one per static point, in place) so that neighbouring normals agree
        /// and the top of every connected piece points up: a deterministic region growing over the k-nearest graph (k in 2..64, no
        /// farther than maxDistance), confident edges first, from at most maxSeeds seeds.  Normals that are not finite or all zero,
        /// and those no seed reached, are left alone.  Returns the stats: rounds, seeds, flipped, unreached, invalid and the
        /// points oriented at each of the four levels.</summary>
        public unsafe long[] OrientNormals (Span<Vector3> normals, int k = 8, float maxDistance = float.PositiveInfinity, int maxSeeds = 64)
        {
            if (k < 2 || k > 64)
                throw new ArgumentOutOfRangeException (nameof (k), "k must be in 2..64");
            if (maxSeeds < 1)
                throw new ArgumentOutOfRangeException (nameof (maxSeeds), "maxSeeds must be at least 1");
            if (normals.Length != TotalPoints)
                throw new ArgumentException ("One normal per static point", nameof (normals));
            var stats = new long[9];
            fixed (Vector3* nrm = normals) fixed (long* st = stats)
                Native.Check (Native.sdfk_points_orient_normals (handle, k, maxDistance, maxSeeds, (float*)nrm, st));
            return stats;
        }

        /// <summary>Extension: one point per occupied voxel of the lattice of edge voxelSize anchored at origin, the centroid of the
        /// voxel's members, voxels in the order of their lowest member.  counts: the members of each voxel; group: per static point
        /// the index of its voxel in the result (for averaging further per-point data; the overload with colors does it on the
        /// device).  A voxelSize below the spacing of the cloud returns the points as they are.  The tree is not changed: make a new KdTree from the result.</summary>
        public unsafe Vector3[] VoxelDownsample (float voxelSize, out int[] counts, out int[] group, Vector3 origin = default)
        {
            if (!(voxelSize > 0) || float.IsInfinity (voxelSize))
                throw new ArgumentOutOfRangeException (nameof (voxelSize), "voxelSize must be finite and positive");
            int n = TotalPoints;
            var points = new Vector3[n];
            var cnt = new int[n];
            group = new int[n];
            long m = 0;
            fixed (Vector3* p = points) fixed (int* c = cnt) fixed (int* g = group)
                Native.Check (Native.sdfk_points_voxel_downsample (handle, voxelSize, (float*)&origin, (float*)p, c, g, &m));
            Array.Resize (ref points, (int)m);
            Array.Resize (ref cnt, (int)m);
            counts = cnt;
            return points;
        }

        /// <summary>Extension: VoxelDownsample with one colour per static point (or a normal, or anything else to average):
        /// colorsOut holds every voxel's mean, summed in the order of the centroid.</summary>
        public unsafe Vector3[] VoxelDownsample (float voxelSize, ReadOnlySpan<Vector3> colors, out int[] counts, out int[] group, out Vector3[] colorsOut,
                                                 Vector3 origin = default)
        {
            if (!(voxelSize > 0) || float.IsInfinity (voxelSize))
                throw new ArgumentOutOfRangeException (nameof (voxelSize), "voxelSize must be finite and positive");
            int n = TotalPoints;
            if (colors.Length != n)
                throw new ArgumentException ("One colour per static point", nameof (colors));
            var points = new Vector3[n];
            var col = new Vector3[n];
            var cnt = new int[n];
            group = new int[n];
            long m = 0;
            fixed (Vector3* ci = colors) fixed (Vector3* p = points) fixed (int* c = cnt) fixed (int* g = group) fixed (Vector3* co = col)
                Native.Check (Native.sdfk_points_voxel_downsample_colors (handle, voxelSize, (float*)&origin, (float*)ci, (float*)p, c, g, (float*)co, &m));
            Array.Resize (ref points, (int)m);
            Array.Resize (ref cnt, (int)m);
            Array.Resize (ref col, (int)m);
            counts = cnt;
            colorsOut = col;
            return points;
        }

        /// <summary>Extension: the colour at every query from colors (one per static point; any three floats -- normals can be
        /// averaged the same way): the blend of the k nearest points' colours (1..64) within maxDistance, weighted as ToVoxels
        /// weights their distances; k = 1: the nearest point's colour.  A query with no point within maxDistance gets (0, 0, 0)
        /// and found 0.  It re-colours the vertices of any mesh from a scan.</summary>
        public unsafe void SampleColors (ReadOnlySpan<Vector3> queries, ReadOnlySpan<Vector3> colors, Span<Vector3> colorsOut, Span<int> found, int k = 8,
                                         float maxDistance = float.PositiveInfinity)
        {
            if (k < 1 || k > 64)
                throw new ArgumentOutOfRangeException (nameof (k), "k must be in 1..64");
            if (colors.Length != TotalPoints)
                throw new ArgumentException ("One colour per static point", nameof (colors));
            if (colorsOut.Length < queries.Length || found.Length < queries.Length)
                throw new ArgumentException ("Output spans are shorter than the queries");
            fixed (Vector3* q = queries) fixed (Vector3* c = colors) fixed (Vector3* o = colorsOut) fixed (int* f = found)
                Native.Check (Native.sdfk_points_blend_colors (handle, (float*)c, (float*)q, queries.Length, k, maxDistance, (float*)o, f));
        }

        /// <summary>Extension: the static points whose mean distance to their k nearest (k in 2..64, the point itself not counted, no
        /// farther than maxDistance) is at most mu + stdRatio * sigma, mu and sigma taken over the cloud.  indices: the kept
        /// indices, ascending; meanDistance: per static point, +inf for an isolated one (no neighbour within maxDistance), which is
        /// never kept; stats: kept, removed, isolated and the bits of mu, sigma and the threshold (BitConverter.Int64BitsToDouble).
        /// The kept points' colours are colors[indices[i]].
        /// The tree is not changed: make a new KdTree from the result.</summary>
        public unsafe Vector3[] RemoveStatisticalOutliers (int k, float stdRatio, out int[] indices, out float[] meanDistance, out long[] stats,
                                                           float maxDistance = float.PositiveInfinity)
        {
            if (k < 2 || k > 64)
                throw new ArgumentOutOfRangeException (nameof (k), "k must be in 2..64");
            if (!(stdRatio >= 0 && stdRatio < float.PositiveInfinity))
                throw new ArgumentOutOfRangeException (nameof (stdRatio), "stdRatio must be finite and not negative");
            int n = TotalPoints;
            var points = new Vector3[n];
            var idx = new int[n];
            meanDistance = new float[n];
            stats = new long[6];
            long kept = 0;
            fixed (Vector3* p = points) fixed (int* i = idx) fixed (float* d = meanDistance) fixed (long* st = stats)
                Native.Check (Native.sdfk_points_outliers (handle, k, stdRatio, maxDistance, d, null, i, (float*)p, &kept, st));
            Array.Resize (ref points, (int)kept);
            Array.Resize (ref idx, (int)kept);
            indices = idx;
            return points;
        }

        /// <summary>Extension: density clustering of the static points (DBSCAN; minPoints = 1: Euclidean cluster extraction).  A point
        /// is core iff at least minPoints static points lie within radius (sqrtf(d2) &lt;= radius, itself and its duplicates included:
        /// counts); clusters are the connected components of the core points, numbered by their lowest core member; any other point
        /// takes the cluster of the core point within radius that is first in (d2, index) order, or is noise, label -1.  sizes: the
        /// members per cluster, core and border; stats: clusters, core, border, noise, hook rounds, shortcut launches.  The result
        /// depends on no order.  The tree is not changed.</summary>
        public unsafe int[] Clusters (float radius, out int[] sizes, out bool[] core, out int[] counts, out long[] stats, int minPoints = 1)
        {
            if (!(radius >= 0))
                throw new ArgumentOutOfRangeException (nameof (radius), "radius must not be negative or NaN");
            if (minPoints < 1)
                throw new ArgumentOutOfRangeException (nameof (minPoints), "minPoints must be at least 1");
            int n = TotalPoints;
            var labels = new int[n];
            var size = new int[n];
            var coreBytes = new byte[n];
            counts = new int[n];
            stats = new long[6];
            long c = 0;
            fixed (int* l = labels) fixed (int* s = size) fixed (byte* cb = coreBytes) fixed (int* cn = counts) fixed (long* st = stats)
                Native.Check (Native.sdfk_points_cluster (handle, radius, minPoints, l, s, cb, cn, &c, st));
            Array.Resize (ref size, (int)c);
            sizes = size;
            core = new bool[n];
            for (int i = 0; i < n; i++)
                core[i] = coreBytes[i] != 0;
            return labels;
        }

        /// <summary>Extension: the static points whose cluster is kept: 0 &lt;= labels[i] &lt; keep.Length and keep[labels[i]].  labels:
        /// one per static point, Clusters' or any other.  indices: the kept indices, ascending; per-point data of the kept points is
        /// data[indices[i]].  Make a new KdTree from the result.</summary>
        public unsafe Vector3[] SelectClusters (ReadOnlySpan<int> labels, ReadOnlySpan<bool> keep, out int[] indices)
        {
            int n = TotalPoints;
            if (labels.Length != n)
                throw new ArgumentException ("One label per static point", nameof (labels));
            var keepBytes = new byte[Math.Max (1, keep.Length)];
            for (int i = 0; i < keep.Length; i++)
                keepBytes[i] = keep[i] ? (byte)1 : (byte)0;
            var points = new Vector3[n];
            var idx = new int[n];
            long kept = 0;
            fixed (int* l = labels) fixed (byte* k = keepBytes) fixed (Vector3* p = points) fixed (int* i = idx)
                Native.Check (Native.sdfk_points_select (handle, l, k, keep.Length, i, (float*)p, &kept));
            Array.Resize (ref points, (int)kept);
            Array.Resize (ref idx, (int)kept);
            indices = idx;
            return points;
        }

        /// <summary>Extension: Clusters, then the points of the clusters of at least minSize members; noise goes.  labels: Clusters'
        /// labels of all static points.</summary>
        public Vector3[] RemoveSmallClusters (float radius, out int[] indices, out int[] labels, int minPoints = 1, int minSize = 2)
        {
            labels = Clusters (radius, out int[] sizes, out _, out _, out _, minPoints);
            var keep = new bool[sizes.Length];
            for (int c = 0; c < keep.Length; c++)
                keep[c] = sizes[c] >= minSize;
            return SelectClusters (labels, keep, out indices);
        }

        /// <summary>Extension: Clusters, then the points of the cluster of greatest size (ties: the lowest number); nothing when there
        /// is no cluster.</summary>
        public Vector3[] LargestCluster (float radius, out int[] indices, int minPoints = 1)
        {
            int[] labels = Clusters (radius, out int[] sizes, out _, out _, out _, minPoints);
            var keep = new bool[sizes.Length];
            int best = 0;
            for (int c = 1; c < sizes.Length; c++)
                if (sizes[c] > sizes[best]) best = c;
            if (keep.Length > 0) keep[best] = true;
            return SelectClusters (labels, keep, out indices);
        }

        /// <summary>Extension: the static points with one outward normal each as a signed distance volume: the blend of the
        /// tangent-plane distances of the k nearest points (1..64) within maxDistance at every cell centre; voxels farther away
        /// get +-maxDistance, the sign carried over from the known ones.  Give a band, then Voxels.Redistance, for a full field.</summary>
        public Voxels ToVoxels (ReadOnlySpan<Vector3> normals, Vector3 min, Vector3 max, int nx, int ny, int nz, int k = 8,
                                float maxDistance = float.PositiveInfinity, bool clipToBounds = false)
        {
            var v = new Voxels (min, max, nx, ny, nz);
            v.SamplePoints (this, normals, k, maxDistance);
            if (clipToBounds) v.ClipToBounds ();
            return v;
        }

        /// <summary>Extension: ToVoxels with one colour per static point: the volume's Colors are SampleColors at every cell centre
        /// (zero where no point lies within maxDistance), which Redistance copies and ToMesh interpolates onto the vertices.</summary>
        public Voxels ToVoxels (ReadOnlySpan<Vector3> normals, ReadOnlySpan<Vector3> colors, Vector3 min, Vector3 max, int nx, int ny, int nz, int k = 8,
                                float maxDistance = float.PositiveInfinity, bool clipToBounds = false)
        {
            var v = new Voxels (min, max, nx, ny, nz);
            v.SamplePoints (this, normals, colors, k, maxDistance);
            if (clipToBounds) v.ClipToBounds ();
            return v;
        }

        public void Dispose ()
        {
            if (handle != IntPtr.Zero) {
                Native.sdfk_points_free (handle);
                handle = IntPtr.Zero;
            }
            GC.SuppressFinalize (this);
        }

        ~KdTree () => Dispose ();
    }

    public partial class Voxels
    {
        /// <summary>Writes the point cloud's signed distance into this volume's device twin; the colours stay what they are.</summary>
        public unsafe void SamplePoints (KdTree points, ReadOnlySpan<Vector3> normals, int k = 8, float maxDistance = float.PositiveInfinity)
        {
            if (normals.Length != points.TotalPoints)
                throw new ArgumentException ("One normal per static point", nameof (normals));
            IntPtr v = hostMayBeNewer ? SyncToDevice () : EnsureDevice (deviceHasColors);
            fixed (Vector3* nrm = normals)
                Native.Check (Native.sdfk_points_to_volume (points.Handle, (float*)nrm, v, k, maxDistance, null));
            deviceIsNewer = true; hostMayBeNewer = false;
        }

        /// <summary>... and its colours from one colour per static point; a device twin without colour storage gets it.</summary>
        public unsafe void SamplePoints (KdTree points, ReadOnlySpan<Vector3> normals, ReadOnlySpan<Vector3> colors, int k = 8,
                                         float maxDistance = float.PositiveInfinity)
        {
            if (normals.Length != points.TotalPoints)
                throw new ArgumentException ("One normal per static point", nameof (normals));
            if (colors.Length != points.TotalPoints)
                throw new ArgumentException ("One colour per static point", nameof (colors));
            EnsureDevice (true);   // (a twin without colour storage is dropped: every voxel of it is written below)
            IntPtr v = hostMayBeNewer ? SyncToDevice () : EnsureDevice (true);
            fixed (Vector3* nrm = normals) fixed (Vector3* col = colors)
                Native.Check (Native.sdfk_points_to_volume_colors (points.Handle, (float*)nrm, (float*)col, v, k, maxDistance, null));
            deviceIsNewer = true; hostMayBeNewer = false;
        }
    }
}
