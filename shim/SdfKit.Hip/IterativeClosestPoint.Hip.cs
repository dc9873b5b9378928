// IterativeClosestPoint.Hip.cs -- SdfKit.IterativeClosestPoint over sdfk_icp_register (include/sdfkit_hip.h).  Replaces
// SdfKit/IterativeClosestPoint.cs with the same public members (IterativeClosestPoint.cs:10-240).  Each iteration is the
// reference's; the reductions and the 3x3 SVD are f64 on the GPU instead of MathNet's float SVD (a stated deviation), every
// later step is the reference's float Matrix4x4 arithmetic.  An empty dynamic set is refused (the reference returns NaN),
// and so is a dynamic point with a NaN or infinite coordinate (the native call checks host points; device points are unchecked).
// Extension: RegisterPoints (points, IcpMetric) and StaticNormals add the point-to-plane metric over sdfk_icp_register_plane; the
// reference's RegisterPoints (points) stays point to point, and so does GlobalRegisterPoints.
// UNCOMPILED HERE (no .NET in the build image); sdfkit_amd/points.py's IterativeClosestPoint is the same layer, tested.
using System;
using System.Linq;
using System.Numerics;
using SdfKit.Hip;

namespace SdfKit
{
    public class IterativeClosestPoint
    {
        readonly KdTree staticTree;

        public int MaxIterations { get; set; } = 100;

        public float GoodCorrespondenceDistance { get; set; } = 0.01f;

        public float ConvergedMaximumTranslation { get; set; } = 1.0e-4f;

        public float ConvergedMaximumRotation { get; set; } = 1.0e-5f;

        public IterativeClosestPoint (ReadOnlySpan<Vector3> staticPoints)
        {
            staticTree = new KdTree (staticPoints);
        }

        public IterativeClosestPoint (ReadOnlyMemory<Vector3>[] staticPoints)
        {
            var n = staticPoints.Length;
            if (n == 0)
                throw new ArgumentException ("At least one set of points must be given", nameof (staticPoints));
            staticTree = new KdTree (staticPoints[0].Span);
            for (int i = 1; i < n; i++)
                staticTree.AddPoints (staticPoints[i].Span);
        }

        public void AddStaticPoints (ReadOnlySpan<Vector3> staticPoints)
        {
            if (staticNormals != null)
                throw new ArgumentException ("AddStaticPoints would leave StaticNormals out of step: pass the new points' normals", nameof (staticPoints));
            staticTree.AddPoints (staticPoints);
        }

        // ---- extension: point to plane (include/sdfkit_hip.h, "IterativeClosestPoint.RegisterPoints, point to plane") ----
        public enum IcpMetric { Auto, Point, Plane }   // Auto: Plane iff StaticNormals is set

        public struct PlaneStats
        {
            public long Kept;        // kept correspondences of the last iteration
            public double SumR2;     // sum of their squared plane distances before the step
            public bool Converged;
            public int Retained;     // eigenvalues of the normal equations the solve retained
        }

        Vector3[]? staticNormals;

        /// <summary>One normal per static point (e.g. from KdTree.EstimateNormals), or null.  With normals set, RegisterPoints
        /// minimises the distances to the tangent planes at the nearest static points.  Their orientation does not matter; a
        /// point whose normal is (0, 0, 0) takes no part.</summary>
        public Vector3[]? StaticNormals {
            get => staticNormals;
            set {
                if (value != null && value.Length != staticTree.TotalPoints)
                    throw new ArgumentException ("One normal per static point must be given", nameof (value));
                staticNormals = value == null ? null : (Vector3[])value.Clone ();
            }
        }

        /// <summary>The stats of the last point-to-plane registration (null after a point-to-point one).</summary>
        public PlaneStats? LastStats { get; private set; }

        public void AddStaticPoints (ReadOnlySpan<Vector3> staticPoints, ReadOnlySpan<Vector3> normals)
        {
            if (staticNormals == null)
                throw new ArgumentException ("Set StaticNormals first", nameof (normals));
            if (normals.Length != staticPoints.Length)
                throw new ArgumentException ("One normal per added point must be given", nameof (normals));
            staticTree.AddPoints (staticPoints);
            var all = new Vector3[staticNormals.Length + normals.Length];
            staticNormals.CopyTo (all, 0);
            normals.CopyTo (all.AsSpan (staticNormals.Length));
            staticNormals = all;
        }

        public unsafe Matrix4x4 RegisterPoints (Span<Vector3> points, IcpMetric metric)
        {
            if (metric == IcpMetric.Point || (metric == IcpMetric.Auto && staticNormals == null)) {
                var t = RegisterPoints (points);
                LastStats = null;
                return t;
            }
            if (staticNormals == null)
                throw new ArgumentException ("IcpMetric.Plane needs StaticNormals", nameof (metric));
            if (staticNormals.Length != staticTree.TotalPoints)
                throw new InvalidOperationException ("StaticNormals is out of step with the static points");
            var prm = new SdfkIcpParams {
                MaxIterations = MaxIterations,
                GoodCorrespondenceDistance = GoodCorrespondenceDistance,
                ConvergedMaximumTranslation = ConvergedMaximumTranslation,
                ConvergedMaximumRotation = ConvergedMaximumRotation,
            };
            Matrix4x4 total;
            long* st = stackalloc long[4];
            fixed (Vector3* p = points)
            fixed (Vector3* nrm = staticNormals)
                Native.Check (Native.sdfk_icp_register_plane (staticTree.Handle, ref prm, (float*)nrm, (float*)p, points.Length, (float*)&total, out _, st));
            LastStats = new PlaneStats { Kept = st[0], SumR2 = BitConverter.Int64BitsToDouble (st[1]), Converged = st[2] != 0, Retained = (int)st[3] };
            return total;
        }

        /// <summary>
        /// Rigidly move the given points to align with the static points
        /// used to construct this instance.
        /// The returned transform is the one used to convert
        /// the given points to their new locations.
        /// </summary>
        public unsafe Matrix4x4 RegisterPoints (Span<Vector3> points)
        {
            var prm = new SdfkIcpParams {
                MaxIterations = MaxIterations,
                GoodCorrespondenceDistance = GoodCorrespondenceDistance,
                ConvergedMaximumTranslation = ConvergedMaximumTranslation,
                ConvergedMaximumRotation = ConvergedMaximumRotation,
            };
            Matrix4x4 total;   // row-major M11..M44: the layout of System.Numerics.Matrix4x4
            fixed (Vector3* p = points)
                Native.Check (Native.sdfk_icp_register (staticTree.Handle, ref prm, (float*)p, points.Length, (float*)&total, out _));
            return total;
        }

        public Matrix4x4[] GlobalRegisterPoints (ReadOnlyMemory<Vector3>[] staticPoints, Memory<Vector3>[] dynamicPoints)
        {
            var n = dynamicPoints.Length;
            if (n == 0) {
                return Array.Empty<Matrix4x4> ();
            }
            var icp = new IterativeClosestPoint (staticPoints);
            var transforms = new Matrix4x4[n];
            for (var i = 0; i < n; i++) {
                var dpoints = dynamicPoints[i].Span;
                transforms[i] = icp.RegisterPoints (dpoints);
                icp.AddStaticPoints (dpoints);
            }
            return transforms;
        }

        public Matrix4x4[] GlobalRegisterPoints (Memory<Vector3>[] points)
        {
            var n = points.Length;
            if (n == 0) {
                return Array.Empty<Matrix4x4> ();
            }
            else if (n == 1) {
                return new Matrix4x4[] { Matrix4x4.Identity };
            }
            var spoints = points.Take (1).Select (x => (ReadOnlyMemory<Vector3>)x).ToArray ();
            var dpoints = points.Skip (1).ToArray ();
            return GlobalRegisterPoints (spoints, dpoints);
        }
    }
}
