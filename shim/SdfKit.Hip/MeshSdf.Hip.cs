// MeshSdf.Hip.cs -- triangle meshes as signed distance fields over sdfk_trimesh_* (include/sdfkit_hip.h).  Not in the reference,
// which converts SDF -> Voxels -> Mesh only: MeshSdf and Mesh.ToVoxels add the way back.  Distances are exact (binary64 closest
// point, ties to the lowest triangle index); the sign is the parity of crossings along z, right for closed meshes.
// UNCOMPILED HERE (no .NET in the build image); sdfkit_amd/meshsdf.py's MeshSdf is the same layer, tested.
using System;
using System.Numerics;
using SdfKit.Hip;

namespace SdfKit
{
    public class MeshSdf : IDisposable
    {
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
    }
}
