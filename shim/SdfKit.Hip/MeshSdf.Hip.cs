// MeshSdf.Hip.cs -- triangle meshes as signed distance fields over sdfk_trimesh_* (include/sdfkit_hip.h).  Not in the reference,
// which converts SDF -> Voxels -> Mesh only: MeshSdf and Mesh.ToVoxels add the way back.  Distances are exact (binary64 closest
// point, ties to the lowest triangle index); the sign is the parity of crossings along z, right for closed meshes.
// SamplePoints (sdfk_trimesh_sample) turns a mesh into a point cloud: points in proportion to area with face normals, colours,
// triangle indices and barycentric weights, one stated function of the mesh, n, the seed and the mode.
// Components / Topology / Select (sdfk_trimesh_components, _topology, _select): the connectivity of the mesh by index -- a label per
// vertex and triangle, a row of integer counts per component, the edge census, and sub-meshes of chosen components.
// Adjacency / Smooth / VertexNormals (sdfk_trimesh_adjacency, _smooth, _vertex_normals): the neighbours of every vertex, Taubin
// smoothing of the positions and area-weighted normals from the geometry; Mesh.Smooth / Mesh.RecomputeNormals on top of them.
// Weld (sdfk_trimesh_weld): the vertices of equal position made one; Mesh.Weld and Concat (a static of the extensions class) on top.
// Simplify (sdfk_trimesh_simplify): vertex clustering, the vertices of one lattice cell made one made vertex; Mesh.Simplify on top.
// RayCast / Occluded / Render / RenderDepth / RenderTriangles (sdfk_trimesh_raycast, _render): the first hit or any hit of arbitrary
// rays, and the mesh as a camera sees it (the ray marcher's camera, light and sky); Mesh.RayCast / Occluded / ToImage on top.
// WindingNumber / Contains / ToVoxels (sign: MeshSign.Winding) (sdfk_trimesh_winding, _to_volume_signed): the generalized winding
// number -- is this point inside, also for meshes with holes or overlapping pieces; Mesh.WindingNumber / Contains on top.
// UNCOMPILED HERE (no .NET in the build image); sdfkit_amd/meshsdf.py's MeshSdf is the same layer, tested.
using System;
using System.Collections.Generic;
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

    /// <summary>MeshSdf.Components: the connected components by index (equal positions with different indices are different
    /// vertices).  Labels are -1 for an unreferenced vertex and an index-degenerate triangle; the per-component arrays have Count
    /// entries; AreaWeights sums the integer sampling weights of the component's triangles.</summary>
    public sealed class MeshComponents
    {
        public long Count;
        public int[] VertexLabels = Array.Empty<int> ();
        public int[] TriangleLabels = Array.Empty<int> ();
        public long[] Triangles = Array.Empty<long> ();
        public long[] Vertices = Array.Empty<long> ();
        public long[] Edges = Array.Empty<long> ();
        public long[] BoundaryEdges = Array.Empty<long> ();
        public long[] NonManifoldEdges = Array.Empty<long> ();
        public long[] OddEdges = Array.Empty<long> ();
        public long[] InconsistentEdges = Array.Empty<long> ();
        public long[] AreaWeights = Array.Empty<long> ();
        public long Rounds, ShortcutLaunches;
        public long EulerCharacteristic (int c) => Vertices[c] - Edges[c] + Triangles[c];
        /// <summary>Every edge is used an even number of times: the condition under which ToVoxels' parity sign is well defined.</summary>
        public bool IsWatertight (int c) => OddEdges[c] == 0;
        public bool IsOriented (int c) => InconsistentEdges[c] == 0 && NonManifoldEdges[c] == 0;
    }

    /// <summary>MeshSdf.Topology: the census of the whole mesh.  Triangles: those that are not index-degenerate; Vertices: referenced.</summary>
    public sealed class MeshTopology
    {
        public long Components, Triangles, Vertices, Edges, BoundaryEdges, NonManifoldEdges, OddEdges, InconsistentEdges, DegenerateTriangles;
        public long EulerCharacteristic => Vertices - Edges + Triangles;
        public bool IsWatertight => OddEdges == 0;
        public bool IsOriented => InconsistentEdges == 0 && NonManifoldEdges == 0;
    }

    /// <summary>MeshSdf.Adjacency: the neighbours of vertex v are Neighbors[Start[v] .. Start[v + 1]), ascending, each once (by
    /// index); Boundary[v] = 1 for the endpoints of an edge with one triangle side.</summary>
    public sealed class MeshAdjacency
    {
        public uint[] Start = Array.Empty<uint> ();
        public uint[] Neighbors = Array.Empty<uint> ();
        public byte[] Boundary = Array.Empty<byte> ();
        public long Degree (int v) => (long)Start[v + 1] - Start[v];
    }

    /// <summary>MeshSdf.Select: the kept vertices' and triangles' old indices, the renumbered index array, positions and colours.</summary>
    /// <summary>MeshSdf.Weld: VertexMap (one per old vertex: the new index of its representative, -1: dropped), the old indices of
    /// the new vertices and of the kept triangles, the renumbered index array, the representatives' own positions and colours
    /// (zeros when the mesh has none), and what went.</summary>
    public sealed class MeshWeld
    {
        public int[] VertexMap = Array.Empty<int> ();
        public int[] VertexIndex = Array.Empty<int> ();
        public int[] TriangleIndex = Array.Empty<int> ();
        public int[] Triangles = Array.Empty<int> ();
        public Vector3[] Vertices = Array.Empty<Vector3> ();
        public Vector3[] Colors = Array.Empty<Vector3> ();
        public long Merged, DegenerateDropped, UnreferencedDropped, Passes;
    }

    /// <summary>MeshSdf.RayCast: per ray the first triangle hit (-1: none), the distance in units of |direction| (+inf: none) and the
    /// barycentric weights of the triangle's three vertices (NaN: none), in MeshSamples' layout.</summary>
    public sealed class MeshRayHits
    {
        public Vector3[] Origins = Array.Empty<Vector3> ();
        public Vector3[] Directions = Array.Empty<Vector3> ();
        public int[] Triangles = Array.Empty<int> ();
        public float[] Distances = Array.Empty<float> ();
        public Vector3[] Weights = Array.Empty<Vector3> ();
        public bool Hit (int i) => Triangles[i] >= 0;
        /// <summary>origin + direction * distance of the hits, in ray order (made on the host).</summary>
        public Vector3[] Points ()
        {
            var p = new List<Vector3> ();
            for (int i = 0; i < Triangles.Length; i++)
                if (Triangles[i] >= 0)
                    p.Add (Origins[i] + Directions[i] * Distances[i]);
            return p.ToArray ();
        }
    }

    /// <summary>MeshSdf.Simplify: MeshWeld's fields for the clustered mesh (VertexMap: the new number of every old vertex's group;
    /// Vertices and Colors: the made ones), the triangles dropped for sharing a vertex set with another, and the kept groups
    /// whose quadric placement fell back to the centroid.</summary>
    public sealed class MeshSimplify
    {
        public int[] VertexMap = Array.Empty<int> ();
        public int[] VertexIndex = Array.Empty<int> ();
        public int[] TriangleIndex = Array.Empty<int> ();
        public int[] Triangles = Array.Empty<int> ();
        public Vector3[] Vertices = Array.Empty<Vector3> ();
        public Vector3[] Colors = Array.Empty<Vector3> ();
        public long Merged, DegenerateDropped, DuplicatesDropped, UnreferencedDropped, Passes, QuadricFallbacks;
    }

    public enum SimplifyPlacement { Representative = 0, Centroid = 1, Quadric = 2 }   // SDFK_SIMPLIFY_REPRESENTATIVE, _CENTROID, _QUADRIC
    public enum SimplifyDuplicates { One = 0, Keep = 1, Cancel = 2 }                    // 0, SDFK_SIMPLIFY_KEEP_DUPLICATES, SDFK_SIMPLIFY_CANCEL_PAIRS

    public sealed class MeshSelection
    {
        public int[] VertexIndex = Array.Empty<int> ();
        public int[] TriangleIndex = Array.Empty<int> ();
        public int[] Triangles = Array.Empty<int> ();
        public Vector3[] Vertices = Array.Empty<Vector3> ();
        public Vector3[] Colors = Array.Empty<Vector3> ();
    }

    public class MeshSdf : IDisposable
    {
        const int SampleStratified = 1;   // SDFK_TRIMESH_SAMPLE_STRATIFIED

        IntPtr handle;   // sdfk_trimesh*
        readonly bool hasColors;
        readonly long vertexCount, triangleCount;

        /// <summary>The triangles of `mesh` (Vertices, Triangles; Colors when any is non-zero).</summary>
        public MeshSdf (Mesh mesh) : this (mesh.Vertices, mesh.Triangles, AnyNonZero (mesh.Colors) ? mesh.Colors : null) { }

        public MeshSdf (ReadOnlySpan<Vector3> vertices, ReadOnlySpan<int> triangles, Vector3[]? colors = null)
        {
            if (colors != null && colors.Length != vertices.Length)
                throw new ArgumentException ("One colour per vertex", nameof (colors));
            Native.EnsureInit ();
            hasColors = colors != null;
            vertexCount = vertices.Length;
            triangleCount = triangles.Length / 3;
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
        /// <summary>sign: MeshSign.Parity (crossings along z: exact on watertight meshes, streaks on others) or MeshSign.Winding
        /// (|WindingNumber| &gt; 1/2 with the acceptance parameter beta: holes are capped by the 1/2 level set and overlapping pieces
        /// are united; the values next to a cap are distances to the mesh's triangles until Voxels.Redistance has run).</summary>
        public Voxels ToVoxels (Vector3 min, Vector3 max, int nx, int ny, int nz, float maxDistance = float.PositiveInfinity, bool clipToBounds = false,
                                MeshSign sign = MeshSign.Parity, float beta = DefaultWindingBeta)
        {
            var v = new Voxels (min, max, nx, ny, nz);
            v.SampleMesh (this, maxDistance, sign, beta);
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

        /// <summary>The connected components by index, with a row of counts each.</summary>
        public unsafe MeshComponents Components ()
        {
            var c = new MeshComponents { VertexLabels = new int[vertexCount], TriangleLabels = new int[triangleCount] };
            long count = 0;
            long* stats = stackalloc long[4];
            long* census = stackalloc long[8];
            fixed (int* vl = c.VertexLabels) fixed (int* tl = c.TriangleLabels)
                Native.Check (Native.sdfk_trimesh_components (handle, vl, tl, &count, stats));
            var rows = new long[count * 8];
            fixed (long* r = rows)
                Native.Check (Native.sdfk_trimesh_topology (handle, census, r, count));
            var cols = new long[8][];
            for (int k = 0; k < 8; k++) {
                cols[k] = new long[count];
                for (long i = 0; i < count; i++)
                    cols[k][i] = rows[8 * i + k];
            }
            c.Count = count;
            c.Triangles = cols[0]; c.Vertices = cols[1]; c.Edges = cols[2]; c.BoundaryEdges = cols[3]; c.NonManifoldEdges = cols[4];
            c.OddEdges = cols[5]; c.InconsistentEdges = cols[6]; c.AreaWeights = cols[7];
            c.Rounds = stats[0]; c.ShortcutLaunches = stats[1];
            return c;
        }

        /// <summary>The edge census of the whole mesh.</summary>
        public unsafe MeshTopology Topology ()
        {
            long* census = stackalloc long[8];
            Native.Check (Native.sdfk_trimesh_topology (handle, census, null, 0));
            return new MeshTopology { Components = census[0], Vertices = census[1], Edges = census[2], BoundaryEdges = census[3],
                                      NonManifoldEdges = census[4], OddEdges = census[5], InconsistentEdges = census[6],
                                      DegenerateTriangles = census[7], Triangles = triangleCount - census[7] };
        }

        /// <summary>The sub-mesh of the components whose flag is set (one flag per component): vertices and triangles keep their
        /// order, triangles are renumbered.</summary>
        public unsafe MeshSelection Select (ReadOnlySpan<bool> keep)
        {
            long count = 0, kv = 0, kt = 0;
            Native.Check (Native.sdfk_trimesh_components (handle, null, null, &count, null));
            if (keep.Length != count)
                throw new ArgumentException ("One flag per component", nameof (keep));
            var k = new byte[keep.Length + 1];   // (never empty: a NULL keep array is refused)
            for (int i = 0; i < keep.Length; i++)
                k[i] = keep[i] ? (byte)1 : (byte)0;
            var vi = new int[vertexCount];
            var ti = new int[triangleCount];
            var tr = new int[triangleCount * 3];
            var vs = new Vector3[vertexCount];
            var cs = new Vector3[vertexCount];
            fixed (byte* kp = k) fixed (int* vip = vi) fixed (int* tip = ti) fixed (int* trp = tr) fixed (Vector3* vsp = vs) fixed (Vector3* csp = cs)
                Native.Check (Native.sdfk_trimesh_select (handle, kp, vip, tip, trp, (float*)vsp, (float*)csp, &kv, &kt));
            return new MeshSelection { VertexIndex = vi.AsSpan (0, (int)kv).ToArray (), TriangleIndex = ti.AsSpan (0, (int)kt).ToArray (),
                                       Triangles = tr.AsSpan (0, (int)kt * 3).ToArray (), Vertices = vs.AsSpan (0, (int)kv).ToArray (),
                                       Colors = cs.AsSpan (0, (int)kv).ToArray () };
        }

        const int SmoothPinBoundary = 1;   // SDFK_TRIMESH_SMOOTH_PIN_BOUNDARY
        const int NormalsFlip = 1;         // SDFK_TRIMESH_NORMALS_FLIP

        /// <summary>The neighbours of every vertex and the boundary bytes; made once per handle and kept on it.</summary>
        public unsafe MeshAdjacency Adjacency ()
        {
            long n = 0;
            Native.Check (Native.sdfk_trimesh_adjacency (handle, null, null, null, &n));
            var a = new MeshAdjacency { Start = new uint[vertexCount + 1], Neighbors = new uint[n], Boundary = new byte[vertexCount] };
            fixed (uint* sp = a.Start) fixed (uint* np = a.Neighbors) fixed (byte* bp = a.Boundary)
                Native.Check (Native.sdfk_trimesh_adjacency (handle, sp, np, bp, null));
            return a;
        }

        /// <summary>The positions after `iterations` iterations of Taubin's lambda | mu smoothing (an iteration is a step with
        /// lambda, then, if mu != 0, a step with mu; mu = 0: plain Laplacian smoothing).  pinBoundary: the vertices of edges with
        /// one triangle side stay.  This handle is not changed.</summary>
        public unsafe Vector3[] Smooth (int iterations, float lambda = 0.5f, float mu = -0.53f, bool pinBoundary = true)
        {
            var o = new Vector3[Math.Max (vertexCount, 1)];
            fixed (Vector3* op = o)
                Native.Check (Native.sdfk_trimesh_smooth (handle, iterations, lambda, mu, pinBoundary ? SmoothPinBoundary : 0, (float*)op));
            return o.AsSpan (0, (int)vertexCount).ToArray ();
        }

        /// <summary>Area-weighted unit vertex normals from the geometry, zeros at a vertex without a triangle that has an area.
        /// positions: one per vertex in place of the handle's own (the output of Smooth, say); empty: the handle's.</summary>
        public unsafe Vector3[] VertexNormals (ReadOnlySpan<Vector3> positions = default, bool flip = false)
        {
            if (positions.Length != 0 && positions.Length != vertexCount)
                throw new ArgumentException ("One position per vertex", nameof (positions));
            var o = new Vector3[Math.Max (vertexCount, 1)];
            fixed (Vector3* pp = positions) fixed (Vector3* op = o)
                Native.Check (Native.sdfk_trimesh_vertex_normals (handle, positions.Length != 0 ? (float*)pp : null, flip ? NormalsFlip : 0, (float*)op));
            return o.AsSpan (0, (int)vertexCount).ToArray ();
        }

        const int WeldKeepDegenerate = 1;     // SDFK_WELD_KEEP_DEGENERATE
        const int WeldKeepUnreferenced = 2;   // SDFK_WELD_KEEP_UNREFERENCED

        /// <summary>The mesh with the vertices of equal position made one.  tolerance 0: equal as values (-0 equals +0); > 0: one
        /// cell of the lattice of that size anchored at the origin (not a ball query: two vertices closer than the tolerance on
        /// opposite sides of a cell face do not weld).  A group becomes its lowest index, which keeps its own position and colour;
        /// triangles that become index-degenerate and representatives no kept triangle names go unless the flags keep them.
        /// This handle is not changed.</summary>
        public unsafe MeshWeld Weld (float tolerance = 0.0f, bool keepDegenerate = false, bool keepUnreferenced = false)
        {
            long kv = 0, kt = 0;
            long* st = stackalloc long[4];
            var vm = new int[vertexCount];
            var vi = new int[vertexCount];
            var ti = new int[triangleCount];
            var tr = new int[triangleCount * 3];
            var vs = new Vector3[vertexCount];
            var cs = new Vector3[vertexCount];
            int flags = (keepDegenerate ? WeldKeepDegenerate : 0) | (keepUnreferenced ? WeldKeepUnreferenced : 0);
            fixed (int* vmp = vm) fixed (int* vip = vi) fixed (int* tip = ti) fixed (int* trp = tr) fixed (Vector3* vsp = vs) fixed (Vector3* csp = cs)
                Native.Check (Native.sdfk_trimesh_weld (handle, tolerance, flags, vmp, vip, tip, trp, (float*)vsp, (float*)csp, &kv, &kt, st));
            return new MeshWeld { VertexMap = vm, VertexIndex = vi.AsSpan (0, (int)kv).ToArray (), TriangleIndex = ti.AsSpan (0, (int)kt).ToArray (),
                                  Triangles = tr.AsSpan (0, (int)kt * 3).ToArray (), Vertices = vs.AsSpan (0, (int)kv).ToArray (),
                                  Colors = cs.AsSpan (0, (int)kv).ToArray (), Merged = st[0], DegenerateDropped = st[1],
                                  UnreferencedDropped = st[2], Passes = st[3] };
        }

        /// <summary>The mesh made smaller by vertex clustering: the vertices of one cell of the lattice of size cellSize anchored at
        /// the origin become one vertex (Quadric: the point nearest the planes of the cell's triangles, kept inside the cell, the
        /// centroid where that fails; Centroid: their mean; Representative: the lowest index as it is).  Triangles that become
        /// index-degenerate go; of those that come to share a vertex set, One keeps the lowest index, Keep all, Cancel the lowest
        /// index of an odd number and none of an even one (a watertight mesh stays watertight).  This handle is not changed.</summary>
        public unsafe MeshSimplify Simplify (float cellSize, SimplifyPlacement placement = SimplifyPlacement.Quadric,
                                             SimplifyDuplicates duplicates = SimplifyDuplicates.One)
        {
            long kv = 0, kt = 0;
            long* st = stackalloc long[6];
            var vm = new int[vertexCount];
            var vi = new int[vertexCount];
            var ti = new int[triangleCount];
            var tr = new int[triangleCount * 3];
            var vs = new Vector3[vertexCount];
            var cs = new Vector3[vertexCount];
            fixed (int* vmp = vm) fixed (int* vip = vi) fixed (int* tip = ti) fixed (int* trp = tr) fixed (Vector3* vsp = vs) fixed (Vector3* csp = cs)
                Native.Check (Native.sdfk_trimesh_simplify (handle, cellSize, (int)placement, (int)duplicates, vmp, vip, tip, trp, (float*)vsp, (float*)csp,
                                                            &kv, &kt, st));
            return new MeshSimplify { VertexMap = vm, VertexIndex = vi.AsSpan (0, (int)kv).ToArray (), TriangleIndex = ti.AsSpan (0, (int)kt).ToArray (),
                                      Triangles = tr.AsSpan (0, (int)kt * 3).ToArray (), Vertices = vs.AsSpan (0, (int)kv).ToArray (),
                                      Colors = cs.AsSpan (0, (int)kv).ToArray (), Merged = st[0], DegenerateDropped = st[1], DuplicatesDropped = st[2],
                                      UnreferencedDropped = st[3], Passes = st[4], QuadricFallbacks = st[5] };
        }

        const int RayAnyHit = 1;   // SDFK_RAY_ANY_HIT

        /// <summary>The first hit of every ray origin + t direction, tMin &lt;= t &lt;= tMax: the watertight ray-triangle test in binary64,
        /// ties to the lowest triangle index.  Directions need not be unit vectors.  A ray with a NaN or infinite component or a zero
        /// direction is a miss.</summary>
        public unsafe MeshRayHits RayCast (ReadOnlySpan<Vector3> origins, ReadOnlySpan<Vector3> directions, float tMin = 0, float tMax = float.PositiveInfinity)
        {
            if (origins.Length != directions.Length)
                throw new ArgumentException ("one origin per direction");
            int n = directions.Length;
            var r = new MeshRayHits { Origins = origins.ToArray (), Directions = directions.ToArray (), Triangles = new int[n], Distances = new float[n],
                                      Weights = new Vector3[n] };
            fixed (Vector3* o = r.Origins) fixed (Vector3* d = r.Directions) fixed (int* t = r.Triangles) fixed (float* dist = r.Distances)
            fixed (Vector3* w = r.Weights)
                Native.Check (Native.sdfk_trimesh_raycast (handle, (float*)o, (float*)d, n, tMin, tMax, 0, t, dist, (float*)w));
            return r;
        }

        /// <summary>Whether anything is hit within the range, per ray (the search stops at the first hit it meets).</summary>
        /// <summary>The smallest beta of the recorded list at which every case of tests/golden/mesh_winding_accuracy.json keeps
        /// every sign.</summary>
        public const float DefaultWindingBeta = 2.5f;

        /// <summary>The generalized winding number of every point (sdfk_trimesh_winding: one stated function of the mesh, the point
        /// and beta): on a closed, consistently oriented mesh 0 outside and +1 or -1 inside, 2 where closed pieces overlap, 0 in a
        /// cavity; smooth where the mesh is open; NaN for a point with a NaN or infinite coordinate.  beta = +inf sums every
        /// triangle.  The hierarchy is made by the handle's first call and kept.</summary>
        public unsafe float[] WindingNumber (ReadOnlySpan<Vector3> points, float beta = DefaultWindingBeta)
        {
            var w = new float[points.Length];
            fixed (Vector3* q = points) fixed (float* o = w)
                Native.Check (Native.sdfk_trimesh_winding (handle, (float*)q, points.Length, beta, o, null));
            return w;
        }

        /// <summary>Whether each point is inside: |winding number| &gt; 1/2, decided in binary64 before the rounding to float.
        /// Independent of which way the normals point; the union of overlapping closed pieces; holes are capped by the 1/2 level
        /// set.</summary>
        public unsafe bool[] Contains (ReadOnlySpan<Vector3> points, float beta = DefaultWindingBeta)
        {
            var b = new byte[points.Length];
            fixed (Vector3* q = points) fixed (byte* o = b)
                Native.Check (Native.sdfk_trimesh_winding (handle, (float*)q, points.Length, beta, null, o));
            var inside = new bool[b.Length];
            for (int i = 0; i < b.Length; i++)
                inside[i] = b[i] != 0;
            return inside;
        }

        /// <summary>WindingNumber / Contains from and into caller-owned device memory (inside: one byte per point; IntPtr.Zero: that
        /// output is not wanted): once the handle has its hierarchy this only queues work on the library stream.</summary>
        public void WindingNumberDevice (IntPtr pointsDev, long n, float beta, IntPtr windingDev, IntPtr insideDev)
        {
            Native.Check (Native.sdfk_trimesh_winding_device (handle, pointsDev, n, beta, windingDev, insideDev));
        }

        public unsafe bool[] Occluded (ReadOnlySpan<Vector3> origins, ReadOnlySpan<Vector3> directions, float tMin = 0, float tMax = float.PositiveInfinity)
        {
            if (origins.Length != directions.Length)
                throw new ArgumentException ("one origin per direction");
            int n = directions.Length;
            var tri = new int[n];
            fixed (Vector3* o = origins) fixed (Vector3* d = directions) fixed (int* t = tri)
                Native.Check (Native.sdfk_trimesh_raycast (handle, (float*)o, (float*)d, n, tMin, tMax, RayAnyHit, t, null, null));
            var occluded = new bool[n];
            for (int i = 0; i < n; i++)
                occluded[i] = tri[i] >= 0;
            return occluded;
        }

        // The camera of RayMarcher.GetCameraRays: the position is the translation of the inverted view transform, the matrix the
        // inverse of view * perspective (System.Numerics, as the reference computes them).
        unsafe void RenderImages (int width, int height, Matrix4x4 viewTransform, float verticalFieldOfViewDegrees, float near, float far,
                                  float* depth, float* rgb, int* triangle)
        {
            Matrix4x4.Invert (viewTransform, out var cam);
            var pos = Vector3.Transform (Vector3.Zero, cam);
            var proj = Matrix4x4.CreatePerspectiveFieldOfView (verticalFieldOfViewDegrees * MathF.PI / 180.0f, (float)width / height, near, far);
            Matrix4x4.Invert (viewTransform * proj, out var vpi);
            Native.Check (Native.sdfk_trimesh_render (handle, width, height, (float*)&pos, (float*)&vpi, near, far, depth, rgb, triangle));
        }

        /// <summary>The mesh as one camera sees it, Lambert-shaded with the ray marcher's light and sky: width * height RGB triples,
        /// row-major.  Vertex colours are blended; a mesh without is white.</summary>
        public unsafe Vector3[] Render (int width, int height, Matrix4x4 viewTransform, float verticalFieldOfViewDegrees = 60, float nearPlaneDistance = 1,
                                        float farPlaneDistance = 100)
        {
            var rgb = new Vector3[width * height];
            fixed (Vector3* p = rgb)
                RenderImages (width, height, viewTransform, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance, null, (float*)p, null);
            return rgb;
        }

        /// <summary>The distance along every pixel's ray to the first surface between the planes, +inf where there is none.</summary>
        public unsafe float[] RenderDepth (int width, int height, Matrix4x4 viewTransform, float verticalFieldOfViewDegrees = 60, float nearPlaneDistance = 1,
                                           float farPlaneDistance = 100)
        {
            var depth = new float[width * height];
            fixed (float* p = depth)
                RenderImages (width, height, viewTransform, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance, p, null, null);
            return depth;
        }

        /// <summary>The triangle every pixel sees, -1 for the sky.</summary>
        public unsafe int[] RenderTriangles (int width, int height, Matrix4x4 viewTransform, float verticalFieldOfViewDegrees = 60, float nearPlaneDistance = 1,
                                             float farPlaneDistance = 100)
        {
            var tri = new int[width * height];
            fixed (int* p = tri)
                RenderImages (width, height, viewTransform, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance, null, null, p);
            return tri;
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
        public void SampleMesh (MeshSdf mesh, float maxDistance = float.PositiveInfinity, MeshSign sign = MeshSign.Parity,
                                float beta = MeshSdf.DefaultWindingBeta)
        {
            IntPtr v = EnsureDevice (mesh.HasColors || deviceHasColors);
            if (sign == MeshSign.Parity)
                Native.Check (Native.sdfk_trimesh_to_volume (mesh.Handle, v, maxDistance));
            else
                Native.Check (Native.sdfk_trimesh_to_volume_signed (mesh.Handle, v, maxDistance, (int)sign, beta));
            deviceIsNewer = true; hostMayBeNewer = false;
        }
    }

    /// <summary>The sign of MeshSdf.ToVoxels: SDFK_TRIMESH_SIGN_PARITY / SDFK_TRIMESH_SIGN_WINDING.</summary>
    public enum MeshSign { Parity = 0, Winding = 1 }

    public static class MeshToVoxelsExtensions
    {
        /// <summary>Mesh.ToVoxels: the mesh as a signed distance volume (MeshSdf.ToVoxels).</summary>
        public static Voxels ToVoxels (this Mesh mesh, Vector3 min, Vector3 max, int nx, int ny, int nz,
                                       float maxDistance = float.PositiveInfinity, bool clipToBounds = false, MeshSign sign = MeshSign.Parity,
                                       float beta = MeshSdf.DefaultWindingBeta)
        {
            using var m = new MeshSdf (mesh);
            return m.ToVoxels (min, max, nx, ny, nz, maxDistance, clipToBounds, sign, beta);
        }

        /// <summary>Mesh.WindingNumber: the generalized winding number of every point (MeshSdf.WindingNumber).</summary>
        public static float[] WindingNumber (this Mesh mesh, ReadOnlySpan<Vector3> points, float beta = MeshSdf.DefaultWindingBeta)
        {
            using var m = new MeshSdf (mesh);
            return m.WindingNumber (points, beta);
        }

        /// <summary>Mesh.Contains: whether each point is inside the mesh, |winding number| &gt; 1/2 (MeshSdf.Contains).</summary>
        public static bool[] Contains (this Mesh mesh, ReadOnlySpan<Vector3> points, float beta = MeshSdf.DefaultWindingBeta)
        {
            using var m = new MeshSdf (mesh);
            return m.Contains (points, beta);
        }

        /// <summary>Mesh.SamplePoints: n points on the mesh in proportion to area (MeshSdf.SamplePoints).</summary>
        public static MeshSamples SamplePoints (this Mesh mesh, long n, ulong seed = 0, bool stratified = true)
        {
            using var m = new MeshSdf (mesh);
            return m.SamplePoints (n, seed, stratified);
        }

        /// <summary>Mesh.Components: the connected components by index with a row of counts each (MeshSdf.Components).</summary>
        public static MeshComponents Components (this Mesh mesh)
        {
            using var m = new MeshSdf (mesh);
            return m.Components ();
        }

        /// <summary>Mesh.Topology: the edge census of the mesh (MeshSdf.Topology).</summary>
        public static MeshTopology Topology (this Mesh mesh)
        {
            using var m = new MeshSdf (mesh);
            return m.Topology ();
        }

        // the vertex normals of `positions` on the side of `present`: flipped iff more vertices have a negative dot product with
        // their present normal than a positive one ((x x' + y y') + z z' in binary64; a tie does not flip)
        static Vector3[] NormalsOnTheSideOf (MeshSdf m, ReadOnlySpan<Vector3> positions, Vector3[] present)
        {
            var n = m.VertexNormals (positions);
            if (present == null || present.Length != n.Length)
                return n;
            long pos = 0, neg = 0;
            for (int i = 0; i < n.Length; i++) {
                double d = ((double)n[i].X * present[i].X + (double)n[i].Y * present[i].Y) + (double)n[i].Z * present[i].Z;
                if (d > 0) pos++;
                if (d < 0) neg++;
            }
            return neg > pos ? m.VertexNormals (positions, true) : n;
        }

        /// <summary>Mesh.Smooth: a new Mesh smoothed by Taubin's lambda | mu (MeshSdf.Smooth); Triangles and Colors copied, Normals
        /// recomputed from the smoothed positions on the side of the present ones (or copied), Min / Max re-measured.</summary>
        public static Mesh Smooth (this Mesh mesh, int iterations = 10, float lambda = 0.5f, float mu = -0.53f, bool pinBoundary = true,
                                   bool normals = true)
        {
            using var m = new MeshSdf (mesh);
            var v = m.Smooth (iterations, lambda, mu, pinBoundary);
            var n = normals ? NormalsOnTheSideOf (m, v, mesh.Normals) : (Vector3[])mesh.Normals.Clone ();
            return new Mesh (v, (Vector3[])mesh.Colors.Clone (), n, (int[])mesh.Triangles.Clone ());   // (the constructor measures Min / Max)
        }

        /// <summary>Mesh.RecomputeNormals: a new Mesh whose Normals are made from the geometry (MeshSdf.VertexNormals).  flip = null
        /// keeps the side of the present normals (marching-cubes meshes wind with their gradient normals: not flipped).</summary>
        public static Mesh RecomputeNormals (this Mesh mesh, bool? flip = null)
        {
            using var m = new MeshSdf (mesh);
            var n = flip.HasValue ? m.VertexNormals (default, flip.Value) : NormalsOnTheSideOf (m, default, mesh.Normals);
            return new Mesh ((Vector3[])mesh.Vertices.Clone (), (Vector3[])mesh.Colors.Clone (), n, (int[])mesh.Triangles.Clone ());
        }

        /// <summary>Mesh.Weld: a new Mesh with the vertices of equal position made one (MeshSdf.Weld): the first step for a triangle
        /// soup or for meshes put together by Concat.  Colors and Normals are gathered from the representatives; normals = true
        /// recomputes Normals from the welded geometry on the side of the gathered ones; Min / Max are re-measured; an empty Mesh
        /// results when nothing is left.</summary>
        public static Mesh Weld (this Mesh mesh, float tolerance = 0.0f, bool normals = false)
        {
            MeshWeld w;
            using (var m = new MeshSdf (mesh))
                w = m.Weld (tolerance);
            var n = new Vector3[w.VertexIndex.Length];
            for (int i = 0; i < n.Length; i++)
                n[i] = mesh.Normals[w.VertexIndex[i]];
            if (normals && n.Length != 0) {
                using var welded = new MeshSdf (w.Vertices, w.Triangles);
                n = NormalsOnTheSideOf (welded, default, n);
            }
            return new Mesh (w.Vertices, w.Colors, n, w.Triangles);   // (the constructor measures Min / Max; empty arrays: an empty Mesh)
        }

        /// <summary>Mesh.Simplify: a new, smaller Mesh by vertex clustering (MeshSdf.Simplify).  Colors come from the call; Normals are
        /// recomputed from the new geometry on the side of the representatives' gathered ones (normals = true) or gathered; Min /
        /// Max are re-measured; an empty Mesh results when nothing is left.</summary>
        public static Mesh Simplify (this Mesh mesh, float cellSize, SimplifyPlacement placement = SimplifyPlacement.Quadric,
                                     SimplifyDuplicates duplicates = SimplifyDuplicates.One, bool normals = true)
        {
            MeshSimplify w;
            using (var m = new MeshSdf (mesh))
                w = m.Simplify (cellSize, placement, duplicates);
            var n = new Vector3[w.VertexIndex.Length];
            for (int i = 0; i < n.Length; i++)
                n[i] = mesh.Normals[w.VertexIndex[i]];
            if (normals && n.Length != 0) {
                using var made = new MeshSdf (w.Vertices, w.Triangles);
                n = NormalsOnTheSideOf (made, default, n);
            }
            return new Mesh (w.Vertices, w.Colors, n, w.Triangles);   // (the constructor measures Min / Max; empty arrays: an empty Mesh)
        }

        /// <summary>Mesh.RayCast: the first hit of every ray with the mesh (MeshSdf.RayCast).  To cast many batches against one
        /// mesh, keep a MeshSdf.</summary>
        public static MeshRayHits RayCast (this Mesh mesh, ReadOnlySpan<Vector3> origins, ReadOnlySpan<Vector3> directions, float tMin = 0,
                                           float tMax = float.PositiveInfinity)
        {
            using var m = new MeshSdf (mesh);
            return m.RayCast (origins, directions, tMin, tMax);
        }

        /// <summary>Mesh.Occluded: whether each ray hits anything within the range (MeshSdf.Occluded).</summary>
        public static bool[] Occluded (this Mesh mesh, ReadOnlySpan<Vector3> origins, ReadOnlySpan<Vector3> directions, float tMin = 0,
                                       float tMax = float.PositiveInfinity)
        {
            using var m = new MeshSdf (mesh);
            return m.Occluded (origins, directions, tMin, tMax);
        }

        /// <summary>Mesh.ToImage: the mesh rendered as SdfEx.ToImage renders an SDF -- the same camera, light, sky and lens --
        /// as a Vec3Data (MeshSdf.Render).</summary>
        public static Vec3Data ToImage (this Mesh mesh, int width, int height, Matrix4x4 viewTransform, float verticalFieldOfViewDegrees = 60,
                                        float nearPlaneDistance = 1, float farPlaneDistance = 100)
        {
            using var m = new MeshSdf (mesh);
            var rgb = m.Render (width, height, viewTransform, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance);
            var image = new Vec3Data (width, height);
            for (int y = 0; y < height; y++)
                for (int x = 0; x < width; x++)
                    image[x, y] = rgb[y * width + x];
            return image;
        }

        public static Vec3Data ToImage (this Mesh mesh, int width, int height, Vector3 cameraPosition, Vector3 cameraTarget, Vector3 cameraUp,
                                        float verticalFieldOfViewDegrees = 60, float nearPlaneDistance = 1, float farPlaneDistance = 100)
            => mesh.ToImage (width, height, Matrix4x4.CreateLookAt (cameraPosition, cameraTarget, cameraUp), verticalFieldOfViewDegrees, nearPlaneDistance,
                             farPlaneDistance);

        /// <summary>Mesh.Concat: the meshes one after the other, the indices of each offset by the vertices before it (on the host;
        /// nothing is merged: Weld afterwards joins the pieces where their positions agree).</summary>
        public static Mesh Concat (IEnumerable<Mesh> meshes)
        {
            var v = new List<Vector3> ();
            var c = new List<Vector3> ();
            var n = new List<Vector3> ();
            var t = new List<int> ();
            foreach (var m in meshes) {
                int offset = v.Count;
                if ((long)offset + m.Vertices.Length >= 1L << 31)
                    throw new ArgumentException ("2^31 vertices or more", nameof (meshes));
                v.AddRange (m.Vertices);
                c.AddRange (m.Colors.Length == m.Vertices.Length ? m.Colors : new Vector3[m.Vertices.Length]);
                n.AddRange (m.Normals.Length == m.Vertices.Length ? m.Normals : new Vector3[m.Vertices.Length]);
                foreach (int i in m.Triangles)
                    t.Add (i + offset);
            }
            return new Mesh (v.ToArray (), c.ToArray (), n.ToArray (), t.ToArray ());
        }

        static Mesh Selected (Mesh mesh, MeshSdf m, ReadOnlySpan<bool> keep)
        {
            var s = m.Select (keep);
            var normals = new Vector3[s.VertexIndex.Length];
            for (int i = 0; i < normals.Length; i++)
                normals[i] = mesh.Normals[s.VertexIndex[i]];
            return new Mesh (s.Vertices, s.Colors, normals, s.Triangles);   // (the constructor measures Min / Max; empty arrays: an empty Mesh)
        }

        /// <summary>Mesh.SelectComponents: the mesh of the components whose flag is set; Normals gathered, Min / Max re-measured.</summary>
        public static Mesh SelectComponents (this Mesh mesh, ReadOnlySpan<bool> keep)
        {
            using var m = new MeshSdf (mesh);
            return Selected (mesh, m, keep);
        }

        /// <summary>Mesh.RemoveSmallComponents: keeps a component iff Triangles >= minTriangles and
        /// (double)AreaWeight >= (double)minAreaFraction * (double)total.</summary>
        public static Mesh RemoveSmallComponents (this Mesh mesh, long minTriangles = 0, float minAreaFraction = 0.0f)
        {
            using var m = new MeshSdf (mesh);
            var c = m.Components ();
            long total = 0;
            foreach (var w in c.AreaWeights) total += w;
            var keep = new bool[c.Count];
            for (int i = 0; i < keep.Length; i++)
                keep[i] = c.Triangles[i] >= minTriangles && (double)c.AreaWeights[i] >= (double)minAreaFraction * (double)total;
            return Selected (mesh, m, keep);
        }

        /// <summary>Mesh.LargestComponent: the greatest AreaWeight; ties go to more triangles, then to the lower number.</summary>
        public static Mesh LargestComponent (this Mesh mesh)
        {
            using var m = new MeshSdf (mesh);
            var c = m.Components ();
            int best = 0;
            for (int i = 1; i < c.Count; i++)
                if (c.AreaWeights[i] != c.AreaWeights[best] ? c.AreaWeights[i] > c.AreaWeights[best] : c.Triangles[i] > c.Triangles[best])
                    best = i;
            var keep = new bool[c.Count];
            if (c.Count > 0) keep[best] = true;
            return Selected (mesh, m, keep);
        }
    }
}
