// MeshSdf.Hip.cs -- triangle meshes as signed distance fields over sdfk_trimesh_* (include/sdfkit_hip.h).  Not in the reference,
// which converts SDF -> Voxels -> Mesh only: MeshSdf and Mesh.ToVoxels add the way back.  Distances are exact (binary64 closest
// point, ties to the lowest triangle index); the sign is the parity of crossings along z, right for closed meshes.
// SamplePoints (sdfk_trimesh_sample) turns a mesh into a point cloud: points in proportion to area with face normals, colours,
// triangle indices and barycentric weights, one stated function of the mesh, n, the seed and the mode.
// UNCOMPILED HERE (no .NET in the build image); sdfkit_amd/meshsdf.py's MeshSdf is the same layer, tested.
using System;
using System.Numerics;
using SdfKit.Hip;

namespace SdfKit
{
    /// <summary>MeshSdf.SamplePoints: per sample the point, the unit face normal, the blended colour (null when the mesh has none),
    /// the triangle and the barycentric weights of its three vertices as the colour blend used them.</summary>
    public sealed class MeshSamples
    {
        public Vector3[] Points = Array.Empty<Vector3> ();
        public Vector3[] Normals = Array.Empty<Vector3> ();
        public Vector3[]? Colors;
        public int[] Triangles = Array.Empty<int> ();
        public Vector3[] Weights = Array.Empty<Vector3> ();
    }

    public class MeshSdf : IDisposable
    {
        const int SampleStratified = 1;   // SDFK_TRIMESH_SAMPLE_STRATIFIED

        IntPtr handle;   // sdfk_trimesh*
        readonly bool hasColors;

        /// <summary>The triangles of `mesh` (Vertices, Triangles; Colors when any is non-zero).</summary>
        public MeshSdf (Mesh mesh) : this (mesh.Vertices, mesh.Triangles, AnyNonZero (mesh.Colors) ? mesh.Colors : null) { }

        public MeshSdf (ReadOnlySpan<Vector3> vertices, ReadOnlySpan<int> triangles, Vector3[]? colors = null)
        {
            if (colors != null && colors.Length != vertices.Length)
                throw new ArgumentException ("One colour per vertex", nameof (colors));
            Native.EnsureInit ();
            hasColors = colors != null;
            unsafe {
                fixed (Vector3* v = vertices) fixed (int* t = triangles) fixed (Vector3* c = colors)
                    Native.Check (Native.sdfk_trimesh_create ((float*)v, vertices.Length, t, triangles.Length, (float*)c, out handle));
            }
        }

        internal IntPtr Handle => handle;
        internal bool HasColors => hasColors;

        static bool AnyNonZero (Vector3[]? c)
        {
            if (c == null) return false;
            foreach (var x in c) if (x != Vector3.Zero) return true;
            return false;
        }

        /// <summary>Every query at once: the nearest triangle (-1 for a NaN / infinite query), its distance and closest point.</summary>
        public unsafe void Search (ReadOnlySpan<Vector3> queries, Span<int> triangles, Span<float> distances, Span<Vector3> closest)
        {
            if (triangles.Length < queries.Length || distances.Length < queries.Length || closest.Length < queries.Length)
                throw new ArgumentException ("Output spans are shorter than the queries");
            fixed (Vector3* q = queries) fixed (int* t = triangles) fixed (float* d = distances) fixed (Vector3* c = closest)
                Native.Check (Native.sdfk_trimesh_closest (handle, (float*)q, queries.Length, t, d, (float*)c));
        }

        /// <summary>The signed distance at the cell centres of Voxels(min, max, nx, ny, nz) (the centres SampleSdf evaluates);
        /// distances above maxDistance become +-maxDistance.  Without a band, large volumes far from a fine mesh are slow.</summary>
        public Voxels ToVoxels (Vector3 min, Vector3 max, int nx, int ny, int nz, float maxDistance = float.PositiveInfinity, bool clipToBounds = false)
        {
            var v = new Voxels (min, max, nx, ny, nz);
            v.SampleMesh (this, maxDistance);
            if (clipToBounds)
                v.ClipToBounds ();
            return v;
        }

        /// <summary>n points on the triangles in proportion to area.  stratified: one sample per equal share of the total area, in
        /// triangle order; otherwise independent draws (sample s does not depend on n).  Normals are the unit face normals of the
        /// winding (b - a) x (c - a).  A triangle below 2^-32 of the largest area is never sampled; a mesh without area is refused.</summary>
        public unsafe MeshSamples SamplePoints (long n, ulong seed = 0, bool stratified = true)
        {
            if (n < 0 || n >= 1L << 31)   // (the library refuses it: nothing is allocated for it first)
                Native.Check (Native.sdfk_trimesh_sample (handle, n, seed, stratified ? SampleStratified : 0, null, null, null, null, null, null));
            var m = n;
            var s = new MeshSamples { Points = new Vector3[m], Normals = new Vector3[m], Colors = hasColors ? new Vector3[m] : null,
                                      Triangles = new int[m], Weights = new Vector3[m] };
            fixed (Vector3* p = s.Points) fixed (Vector3* nr = s.Normals) fixed (Vector3* c = s.Colors) fixed (int* t = s.Triangles)
            fixed (Vector3* w = s.Weights)
                Native.Check (Native.sdfk_trimesh_sample (handle, n, seed, stratified ? SampleStratified : 0, (float*)p, (float*)nr, (float*)c, t,
                                                          (float*)w, null));
            return s;
        }

        public void Dispose ()
        {
            if (handle != IntPtr.Zero) {
                Native.sdfk_trimesh_free (handle);
                handle = IntPtr.Zero;
            }
            GC.SuppressFinalize (this);
        }

        ~MeshSdf () => Dispose ();
    }

    public partial class Voxels
    {
        /// <summary>Writes the mesh's signed distance (and blended vertex colours) into this volume's device twin.</summary>
        public void SampleMesh (MeshSdf mesh, float maxDistance = float.PositiveInfinity)
        {
            Native.Check (Native.sdfk_trimesh_to_volume (mesh.Handle, EnsureDevice (mesh.HasColors || deviceHasColors), maxDistance));
            deviceIsNewer = true; hostMayBeNewer = false;
        }
    }

    public static class MeshToVoxelsExtensions
    {
        /// <summary>Mesh.ToVoxels: the mesh as a signed distance volume (MeshSdf.ToVoxels).</summary>
        public static Voxels ToVoxels (this Mesh mesh, Vector3 min, Vector3 max, int nx, int ny, int nz,
                                       float maxDistance = float.PositiveInfinity, bool clipToBounds = false)
        {
            using var m = new MeshSdf (mesh);
            return m.ToVoxels (min, max, nx, ny, nz, maxDistance, clipToBounds);
        }

        /// <summary>Mesh.SamplePoints: n points on the mesh in proportion to area (MeshSdf.SamplePoints).</summary>
        public static MeshSamples SamplePoints (this Mesh mesh, long n, ulong seed = 0, bool stratified = true)
        {
            using var m = new MeshSdf (mesh);
            return m.SamplePoints (n, seed, stratified);
        }
    }
}
