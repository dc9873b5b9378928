// DepthFusion.Hip.cs -- depth frames into volumes and points over libsdfkit_hip.so (include/sdfkit_hip.h, "Depth images: fusion and
// unprojection").  A depth frame is what RayMarcher.RenderDepth and MeshSdf.RenderDepth make: the distance along every pixel's ray,
// row-major, +inf where nothing was seen.
// DepthFusion (sdfk_volume_integrate_depth): a running weighted average of truncated signed distances (Curless and Levoy 1996) in
// two Voxels, Values and Weights; Redistance and ToMesh turn it into a surface.
// DepthFusion.ToPoints (sdfk_depth_unproject): a frame as points, camera + ray * depth, for KdTree / IterativeClosestPoint.
// UNCOMPILED HERE (no .NET in the build image); sdfkit_amd/fusion.py's DepthFusion / DepthToPoints is the same layer, tested.
using System;
using System.Numerics;
using SdfKit.Hip;

namespace SdfKit
{
    /// <summary>The counts of one Integrate: voxels updated; of them, surface observations within the truncation; of them, first
    /// observations; pixels with a depth in range.</summary>
    public struct DepthFusionStats
    {
        public long Updated, Surface, First, ValidPixels;
    }

    /// <summary>DepthToPoints: per valid pixel, in pixel order, the point, the gathered colour (null without rgb) and j * width + i.</summary>
    public sealed class DepthPoints
    {
        public Vector3[] Points = Array.Empty<Vector3> ();
        public Vector3[]? Colors;
        public int[] Pixels = Array.Empty<int> ();
    }

    /// <summary>The unseen convention: a voxel no frame has observed keeps <c>unseen</c>.  With the default -truncation and carve
    /// (a pixel that saw nothing within depthMax frees the space along its ray) unseen space is solid and seen-empty space is free,
    /// so a fully scanned object meshes watertight; unseen = +truncation without carving is the classic open surface, with a
    /// spurious sheet one truncation behind every observed surface.</summary>
    public sealed class DepthFusion
    {
        public readonly float Truncation, Unseen, MaxWeight;
        public readonly bool Carve;
        public int Frames { get; private set; }
        public readonly Voxels Values, Weights;

        public DepthFusion (Vector3 min, Vector3 max, int nx, int ny, int nz, float truncation, float? unseen = null, bool carve = true,
                            float maxWeight = float.PositiveInfinity)
        {
            Truncation = truncation;
            Unseen = unseen ?? -truncation;
            Carve = carve;
            MaxWeight = maxWeight;
            Values = new Voxels (min, max, nx, ny, nz);
            Weights = new Voxels (min, max, nx, ny, nz);
            var v = Values.Values;   // (the managed array: uploaded by the first Integrate)
            for (int i = 0; i < nx; i++)
                for (int j = 0; j < ny; j++)
                    for (int k = 0; k < nz; k++)
                        v[i, j, k] = Unseen;
            _ = Weights.Values;      // zeros
        }

        static void Camera (int width, int height, Matrix4x4 viewTransform, float fov, float near, float far, out Vector3 pos, out Matrix4x4 vp,
                            out Matrix4x4 vpi)
        {
            Matrix4x4.Invert (viewTransform, out var cam);
            pos = Vector3.Transform (Vector3.Zero, cam);
            var proj = Matrix4x4.CreatePerspectiveFieldOfView (fov * MathF.PI / 180.0f, (float)width / height, near, far);
            vp = viewTransform * proj;
            Matrix4x4.Invert (vp, out vpi);
        }

        SdfkFusionParams Params (float weight, float depthMin, float depthMax) => new SdfkFusionParams {
            Truncation = Truncation, DepthMin = depthMin, DepthMax = depthMax, Weight = weight, MaxWeight = MaxWeight, Flags = Carve ? 1 : 0 };

        /// <summary>One frame into the average, seen by the camera it was rendered with (the ray marcher's lens and defaults).
        /// depthMin / depthMax: the range of depths that are observations (null: the near / the far plane).</summary>
        public unsafe DepthFusionStats Integrate (float[] depth, int width, int height, Matrix4x4 viewTransform, float weight = 1, float? depthMin = null,
                                                  float? depthMax = null, float verticalFieldOfViewDegrees = 60, float nearPlaneDistance = 1,
                                                  float farPlaneDistance = 100)
        {
            if (depth.Length != width * height) throw new ArgumentException ("depth is not width * height long", nameof (depth));
            Camera (width, height, viewTransform, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance, out var pos, out var vp, out _);
            var prm = Params (weight, depthMin ?? nearPlaneDistance, depthMax ?? farPlaneDistance);
            var st = stackalloc long[4];
            IntPtr hv = Values.SyncToDevice (), hw = Weights.SyncToDevice ();
            fixed (float* d = depth)
                Native.Check (Native.sdfk_volume_integrate_depth (hv, hw, d, width, height, (float*)&pos, (float*)&vp, &prm, st));
            return Done (st);
        }

        /// <summary>From a depth image in device memory, queued on the library stream: the camera position and the FORWARD
        /// view-projection (viewTransform * projection, the matrix whose inverse the renders take).</summary>
        public unsafe DepthFusionStats IntegrateDevice (IntPtr depthDev, int width, int height, Vector3 cameraPosition, Matrix4x4 viewProjection,
                                                        float depthMin, float depthMax, float weight = 1)
        {
            var prm = Params (weight, depthMin, depthMax);
            var st = stackalloc long[4];
            IntPtr hv = Values.SyncToDevice (), hw = Weights.SyncToDevice ();
            Native.Check (Native.sdfk_volume_integrate_depth_device (hv, hw, depthDev, width, height, (float*)&cameraPosition, (float*)&viewProjection,
                                                                     &prm, st));
            return Done (st);
        }

        unsafe DepthFusionStats Done (long* st)
        {
            Values.DeviceWritten ();
            Weights.DeviceWritten ();
            Frames++;
            return new DepthFusionStats { Updated = st[0], Surface = st[1], First = st[2], ValidPixels = st[3] };
        }

        /// <summary>The averaged values as they are: projective, truncated distances; unseen voxels hold <c>Unseen</c>.</summary>
        public Voxels ToVoxels () => Values;

        /// <summary>The surface of the fused volume; redistance: through Voxels.Redistance first, which makes distances of the
        /// projective, clamped values.</summary>
        public Mesh ToMesh (float isoValue = 0, bool redistance = true) => (redistance ? Values.Redistance (isoValue) : Values).ToMesh (isoValue);

        /// <summary>A depth frame as points: camera + ray * depth for every pixel with depthMin &lt;= depth &lt;= depthMax (null: the
        /// near / the far plane), in pixel order -- for a frame MeshSdf.RenderDepth made, that render's hit points bit for bit.</summary>
        public static unsafe DepthPoints ToPoints (float[] depth, int width, int height, Matrix4x4 viewTransform, Vector3[]? rgb = null,
                                                   float? depthMin = null, float? depthMax = null, float verticalFieldOfViewDegrees = 60,
                                                   float nearPlaneDistance = 1, float farPlaneDistance = 100)
        {
            if (depth.Length != width * height) throw new ArgumentException ("depth is not width * height long", nameof (depth));
            if (rgb != null && rgb.Length != depth.Length) throw new ArgumentException ("rgb is not the depth image's size", nameof (rgb));
            Native.EnsureInit ();
            Camera (width, height, viewTransform, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance, out var pos, out _, out var vpi);
            var pts = new Vector3[depth.Length];
            var cols = rgb != null ? new Vector3[depth.Length] : null;
            var pix = new int[depth.Length];
            long n;
            fixed (float* d = depth) fixed (Vector3* c = rgb) fixed (Vector3* p = pts) fixed (Vector3* o = cols) fixed (int* x = pix)
                Native.Check (Native.sdfk_depth_unproject (d, (float*)c, width, height, (float*)&pos, (float*)&vpi, depthMin ?? nearPlaneDistance,
                                                           depthMax ?? farPlaneDistance, (float*)p, (float*)o, x, out n));
            Array.Resize (ref pts, (int)n);
            Array.Resize (ref pix, (int)n);
            if (cols != null) Array.Resize (ref cols, (int)n);
            return new DepthPoints { Points = pts, Colors = cols, Pixels = pix };
        }
    }
}
