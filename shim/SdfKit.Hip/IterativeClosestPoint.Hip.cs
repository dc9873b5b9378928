// IterativeClosestPoint.Hip.cs -- SdfKit.IterativeClosestPoint over sdfk_icp_register (include/sdfkit_hip.h).  Replaces
// SdfKit/IterativeClosestPoint.cs with the same public members (IterativeClosestPoint.cs:10-240).  Each iteration is the
// reference's; the reductions and the 3x3 SVD are f64 on the GPU instead of MathNet's float SVD (a stated deviation), every
// later step is the reference's float Matrix4x4 arithmetic.  An empty dynamic set is refused (the reference returns NaN),
// and so is a dynamic point with a NaN or infinite coordinate (the native call checks host points; device points are unchecked).
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
            staticTree.AddPoints (staticPoints);
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
