// Native.cs -- P/Invoke surface of libsdfkit_hip.so (include/sdfkit_hip.h), one [DllImport] per entry point the
// shim uses.  UNCOMPILED IN THIS REPOSITORY: the build image has no .NET toolchain (DESIGN.md section 1); the same
// ABI is driven end to end by the ctypes mirror sdfkit_amd/_native.py, whose SIGNATURES table this file follows
// entry for entry (tests/test_abi.py checks header <-> exports <-> ctypes table).
using System;
using System.Numerics;
using System.Runtime.InteropServices;

namespace SdfKit.Hip
{
    /// <summary>struct sdfk_op (include/sdfkit_hip.h): one float32 SSA instruction; value id = index.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SdfkOp
    {
        public int Opcode, A, B, C, D;
        public float Imm;
    }

    /// <summary>struct sdfk_fusion_params (include/sdfkit_hip.h)</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SdfkFusionParams
    {
        public float Truncation, DepthMin, DepthMax, Weight, MaxWeight;
        public int Flags;   // SDFK_FUSE_CARVE_BEYOND = 1
    }

    /// <summary>struct sdfk_icp_params (include/sdfkit_hip.h)</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SdfkIcpParams
    {
        public int MaxIterations;
        public float GoodCorrespondenceDistance, ConvergedMaximumTranslation, ConvergedMaximumRotation;
    }

    /// <summary>enum sdfk_opcode</summary>
    public enum Op
    {
        Const = 0, X = 1, Y = 2, Z = 3, Add = 4, Sub = 5, Mul = 6, Div = 7, Neg = 8, Abs = 9, Sqrt = 10, Floor = 11,
        MinSel = 12, MaxSel = 13, MinIeee = 14, MaxIeee = 15, SelLt = 16,
        VoxelNearest = 17, VoxelLinear = 18,   // reads of a bound volume: D = (slot << 2) | channel (3 = distance)
        Sin = 19, Cos = 20, Exp = 21, Log = 22, Atan2 = 23,   // MathF.Sin / Cos / Exp / Log / Atan2(y = A, x = B): faithful float32 functions
    }

    static unsafe class Native
    {
        const string Lib = "sdfkit_hip";   // libsdfkit_hip.so next to the assembly or on LD_LIBRARY_PATH

        // lifetime
        [DllImport(Lib)] public static extern int sdfk_abi_version();
        [DllImport(Lib)] public static extern int sdfk_init(int device);
        [DllImport(Lib)] public static extern void sdfk_shutdown();
        [DllImport(Lib)] public static extern int sdfk_synchronize();
        [DllImport(Lib)] public static extern IntPtr sdfk_last_error();
        // programs (Sdf delegate / SdfExprCompiler.Compile, Sdf.cs:8, SdfExpr.cs:225-273)
        [DllImport(Lib)] public static extern int sdfk_program_create(SdfkOp* ops, int nOps, int* outRgbw, int writesColor, out IntPtr program);
        [DllImport(Lib)] public static extern int sdfk_program_check(SdfkOp* ops, int nOps, int* outRgbw, int writesColor);
        [DllImport(Lib)] public static extern int sdfk_program_create_bound(SdfkOp* ops, int nOps, int* outRgbw, int writesColor, IntPtr* volumes, int nVolumes, out IntPtr program);
        [DllImport(Lib)] public static extern int sdfk_program_check_bound(SdfkOp* ops, int nOps, int* outRgbw, int writesColor, int nVolumes);
        [DllImport(Lib)] public static extern void sdfk_program_destroy(IntPtr program);
        // Voxels (Voxels.cs)
        [DllImport(Lib)] public static extern int sdfk_volume_create(int nx, int ny, int nz, float* min, float* max, int withColors, out IntPtr volume);
        [DllImport(Lib)] public static extern int sdfk_volume_upload(IntPtr volume, float* values, float* colors3);
        [DllImport(Lib)] public static extern int sdfk_volume_download(IntPtr volume, float* values, float* colors3);
        [DllImport(Lib)] public static extern int sdfk_volume_clip_to_bounds(IntPtr volume);
        [DllImport(Lib)] public static extern void sdfk_volume_free(IntPtr volume);
        [DllImport(Lib)] public static extern int sdfk_sample(IntPtr program, IntPtr volume, int clipToBounds);
        // MarchingCubes.CreateMesh (MarchingCubes.cs:39-92), SdfEx.ToMesh (Sdf.cs:59-63)
        [DllImport(Lib)] public static extern int sdfk_march(IntPtr volume, float iso, int step, out IntPtr mesh);
        [DllImport(Lib)] public static extern int sdfk_march_host(float* values, float* colors3, int nx, int ny, int nz, float* min, float* max, float iso, int step, out IntPtr mesh);
        [DllImport(Lib)] public static extern int sdfk_sample_march(IntPtr program, float* min, float* max, int nx, int ny, int nz, int clip, float iso, int step, out IntPtr mesh);
        // Mesh (Mesh.cs)
        [DllImport(Lib)] public static extern int sdfk_mesh_counts(IntPtr mesh, out long nVertices, out long nIndices);
        [DllImport(Lib)] public static extern int sdfk_mesh_bounds(IntPtr mesh, float* min, float* max);
        [DllImport(Lib)] public static extern int sdfk_mesh_copy(IntPtr mesh, float* v, float* c, float* n, int* tri);
        [DllImport(Lib)] public static extern void sdfk_mesh_free(IntPtr mesh);
        [DllImport(Lib)] public static extern int sdfk_mesh_size_hint(IntPtr mesh, out long nVertices, out long nIndices, out int exact);
        [DllImport(Lib)] public static extern int sdfk_mesh_transform(IntPtr mesh, float* matrix16, float* normalMatrix16);
        [DllImport(Lib)] public static extern int sdfk_host_prefault(void* p, long nBytes);
        // options (what used to be environment variables): enum sdfk_option
        [DllImport(Lib)] public static extern int sdfk_set_option(int key, long value);
        [DllImport(Lib)] public static extern int sdfk_get_option(int key, out long value);
        [DllImport(Lib)] public static extern int sdfk_set_cache_dir([MarshalAs(UnmanagedType.LPStr)] string path);
        [DllImport(Lib)] public static extern int sdfk_stream_placement(int* out8);   // diagnostics: which streams run side by side
        // Z-slab sharding over the GPUs of one node, one process per GPU (SdfEx.ToMesh, Sdf.cs:59-63): Dist.cs
        [DllImport(Lib)] public static extern int sdfk_dist_unique_id(byte* id128);
        [DllImport(Lib)] public static extern int sdfk_dist_init(int world, int rank, byte* id128);
        [DllImport(Lib)] public static extern int sdfk_dist_info(out int world, out int rank, out int backend);
        [DllImport(Lib)] public static extern void sdfk_dist_shutdown();
        [DllImport(Lib)] public static extern int sdfk_dist_to_mesh(IntPtr program, float* min, float* max, int nx, int ny, int nz, int clip, float iso, out IntPtr mesh);
        [DllImport(Lib)] public static extern int sdfk_dist_session_create(IntPtr program, float* min, float* max, int nx, int ny, int nz, int clip, float iso, int depth, out IntPtr session);
        [DllImport(Lib)] public static extern int sdfk_dist_submit(IntPtr session);
        [DllImport(Lib)] public static extern int sdfk_dist_collect(IntPtr session, out long nVerticesMine, out long nIndicesMine);
        [DllImport(Lib)] public static extern int sdfk_dist_counts(IntPtr session, long* counts2PerRank);
        [DllImport(Lib)] public static extern int sdfk_dist_mesh(IntPtr session, out IntPtr mesh);
        [DllImport(Lib)] public static extern int sdfk_dist_tune(IntPtr session, int stepsPerMode, long* nsPerConfig4);
        [DllImport(Lib)] public static extern int sdfk_dist_stats(IntPtr session, long* stats8);
        [DllImport(Lib)] public static extern int sdfk_dist_slab_mesh(IntPtr session, out IntPtr mesh);
        [DllImport(Lib)] public static extern void sdfk_dist_session_free(IntPtr session);
        [DllImport(Lib)] public static extern int sdfk_eval_points(IntPtr program, float* points3, long n, float* rgbw4);   // SdfEx.Sample, Sdf.cs:22-47
        // KdTree.cs / IterativeClosestPoint.cs (KdTree.Hip.cs, IterativeClosestPoint.Hip.cs)
        [DllImport(Lib)] public static extern int sdfk_points_create(float* points3, long n, out IntPtr points);
        [DllImport(Lib)] public static extern int sdfk_points_create_device(IntPtr points3Dev, long n, out IntPtr points);
        [DllImport(Lib)] public static extern int sdfk_points_add(IntPtr points, float* points3, long n);
        [DllImport(Lib)] public static extern int sdfk_points_add_device(IntPtr points, IntPtr points3Dev, long n);
        [DllImport(Lib)] public static extern int sdfk_points_count(IntPtr points, out long n);
        [DllImport(Lib)] public static extern int sdfk_points_search(IntPtr points, float* queries3, long n, int* index, float* distance, float* nearest3);
        [DllImport(Lib)] public static extern int sdfk_points_search_device(IntPtr points, IntPtr queries3Dev, long n, IntPtr indexDev, IntPtr distanceDev,
                                                                            IntPtr nearest3Dev);
        [DllImport(Lib)] public static extern int sdfk_points_stats(IntPtr points, long* stats5);
        [DllImport(Lib)] public static extern int sdfk_points_knn(IntPtr points, float* queries3, long n, int k, float maxDistance, int* index, float* distance, int* found);
        [DllImport(Lib)] public static extern int sdfk_points_knn_device(IntPtr points, IntPtr queries3Dev, long n, int k, float maxDistance, IntPtr indexDev,
                                                                         IntPtr distanceDev, IntPtr foundDev);
        [DllImport(Lib)] public static extern int sdfk_points_radius_count(IntPtr points, float* queries3, long n, float radius, long* offsets);
        [DllImport(Lib)] public static extern int sdfk_points_radius_count_device(IntPtr points, IntPtr queries3Dev, long n, float radius, IntPtr offsetsDev);
        [DllImport(Lib)] public static extern int sdfk_points_radius_fill(IntPtr points, float* queries3, long n, float radius, long* offsets, int* index, float* distance);
        [DllImport(Lib)] public static extern int sdfk_points_radius_fill_device(IntPtr points, IntPtr queries3Dev, long n, float radius, IntPtr offsetsDev,
                                                                                 IntPtr indexDev, IntPtr distanceDev);
        // point clouds: normals and signed distance volumes (KdTree.Hip.cs)
        [DllImport(Lib)] public static extern int sdfk_points_normals(IntPtr points, int k, float maxDistance, float* viewpoints3, long nViewpoints, float* normals3,
                                                                      float* variation);
        [DllImport(Lib)] public static extern int sdfk_points_normals_device(IntPtr points, int k, float maxDistance, IntPtr viewpoints3Dev, long nViewpoints,
                                                                             IntPtr normals3Dev, IntPtr variationDev);
        [DllImport(Lib)] public static extern int sdfk_points_to_volume(IntPtr points, float* normals3, IntPtr volume, int k, float maxDistance, long* stats4);
        [DllImport(Lib)] public static extern int sdfk_points_to_volume_device(IntPtr points, IntPtr normals3Dev, IntPtr volume, int k, float maxDistance,
                                                                               long* stats4);
        [DllImport(Lib)] public static extern int sdfk_points_orient_normals(IntPtr points, int k, float maxDistance, int maxSeeds, float* normals3, long* stats9);
        [DllImport(Lib)] public static extern int sdfk_points_orient_normals_device(IntPtr points, int k, float maxDistance, int maxSeeds, IntPtr normals3Dev,
                                                                                    long* stats9);
        [DllImport(Lib)] public static extern int sdfk_points_voxel_downsample(IntPtr points, float voxelSize, float* origin3, float* pointsOut, int* counts, int* group, long* m);
        [DllImport(Lib)] public static extern int sdfk_points_voxel_downsample_device(IntPtr points, float voxelSize, float* origin3, IntPtr pointsOutDev, IntPtr countsDev,
            IntPtr groupDev, long* m);
        [DllImport(Lib)] public static extern int sdfk_points_outliers(IntPtr points, int k, float stdRatio, float maxDistance, float* meanDistance, byte* keep, int* indexOut,
            float* pointsOut, long* nKept, long* stats6);
        [DllImport(Lib)] public static extern int sdfk_points_outliers_device(IntPtr points, int k, float stdRatio, float maxDistance, IntPtr meanDistanceDev, IntPtr keepDev,
            IntPtr indexOutDev, IntPtr pointsOutDev, long* nKept, long* stats6);
        // point clouds: clusters (KdTree.Hip.cs)
        [DllImport(Lib)] public static extern int sdfk_points_cluster(IntPtr points, float radius, int minPoints, int* labels, int* sizes, byte* core, int* counts,
            long* nClusters, long* stats6);
        [DllImport(Lib)] public static extern int sdfk_points_cluster_device(IntPtr points, float radius, int minPoints, IntPtr labelsDev, IntPtr sizesDev, IntPtr coreDev,
            IntPtr countsDev, long* nClusters, long* stats6);
        [DllImport(Lib)] public static extern int sdfk_points_select(IntPtr points, int* labels, byte* keep, long nClusters, int* indexOut, float* pointsOut, long* nKept);
        [DllImport(Lib)] public static extern int sdfk_points_select_device(IntPtr points, IntPtr labelsDev, IntPtr keepDev, long nClusters, IntPtr indexOutDev,
            IntPtr pointsOutDev, long* nKept);
        // point clouds: per-point colours (KdTree.Hip.cs)
        [DllImport(Lib)] public static extern int sdfk_points_blend_colors(IntPtr points, float* colors3, float* queries3, long nQueries, int k, float maxDistance,
            float* colorsOut, int* found);
        [DllImport(Lib)] public static extern int sdfk_points_blend_colors_device(IntPtr points, IntPtr colors3Dev, IntPtr queries3Dev, long nQueries, int k,
            float maxDistance, IntPtr colorsOutDev, IntPtr foundDev);
        [DllImport(Lib)] public static extern int sdfk_points_to_volume_colors(IntPtr points, float* normals3, float* colors3, IntPtr volume, int k, float maxDistance,
            long* stats4);
        [DllImport(Lib)] public static extern int sdfk_points_to_volume_colors_device(IntPtr points, IntPtr normals3Dev, IntPtr colors3Dev, IntPtr volume, int k,
            float maxDistance, long* stats4);
        [DllImport(Lib)] public static extern int sdfk_points_voxel_downsample_colors(IntPtr points, float voxelSize, float* origin3, float* colors3, float* pointsOut,
            int* counts, int* group, float* colorsOut, long* m);
        [DllImport(Lib)] public static extern int sdfk_points_voxel_downsample_colors_device(IntPtr points, float voxelSize, float* origin3, IntPtr colors3Dev,
            IntPtr pointsOutDev, IntPtr countsDev, IntPtr groupDev, IntPtr colorsOutDev, long* m);
        [DllImport(Lib)] public static extern void sdfk_points_free(IntPtr points);
        [DllImport(Lib)] public static extern int sdfk_icp_register(IntPtr points, ref SdfkIcpParams prm, float* points3, long n, float* total16, out int iterations);
        [DllImport(Lib)] public static extern int sdfk_icp_register_device(IntPtr points, ref SdfkIcpParams prm, IntPtr points3Dev, long n, float* total16,
                                                                           out int iterations);
        [DllImport(Lib)] public static extern int sdfk_icp_register_plane(IntPtr points, ref SdfkIcpParams prm, float* normals3, float* points3, long n,
                                                                          float* total16, out int iterations, long* stats4);
        [DllImport(Lib)] public static extern int sdfk_icp_register_plane_device(IntPtr points, ref SdfkIcpParams prm, IntPtr normals3Dev, IntPtr points3Dev,
                                                                                 long n, float* total16, out int iterations, long* stats4);
        // triangle-mesh distance (MeshSdf.Hip.cs)
        [DllImport(Lib)] public static extern int sdfk_trimesh_create(float* vertices3, long nVertices, int* triangles, long nIndices, float* colors3,
                                                                      out IntPtr trimesh);
        [DllImport(Lib)] public static extern int sdfk_trimesh_create_device(IntPtr vertices3Dev, long nVertices, IntPtr trianglesDev, long nIndices,
                                                                             IntPtr colors3Dev, out IntPtr trimesh);
        [DllImport(Lib)] public static extern int sdfk_trimesh_closest(IntPtr trimesh, float* queries3, long n, int* triangle, float* distance, float* closest3);
        [DllImport(Lib)] public static extern int sdfk_trimesh_closest_device(IntPtr trimesh, IntPtr queries3Dev, long n, IntPtr triangleDev,
                                                                              IntPtr distanceDev, IntPtr closest3Dev);
        [DllImport(Lib)] public static extern int sdfk_trimesh_to_volume(IntPtr trimesh, IntPtr volume, float maxDistance);
        [DllImport(Lib)] public static extern int sdfk_trimesh_stats(IntPtr trimesh, long* stats8);
        [DllImport(Lib)] public static extern int sdfk_trimesh_sample(IntPtr trimesh, long n, ulong seed, int flags, float* points3, float* normals3,
                                                                      float* colors3, int* triangle, float* weights3, long* stats2);
        [DllImport(Lib)] public static extern int sdfk_trimesh_sample_device(IntPtr trimesh, long n, ulong seed, int flags, IntPtr points3Dev,
                                                                             IntPtr normals3Dev, IntPtr colors3Dev, IntPtr triangleDev, IntPtr weights3Dev,
                                                                             long* stats2);
        [DllImport(Lib)] public static extern int sdfk_trimesh_components(IntPtr trimesh, int* vertexComponent, int* triangleComponent, long* nComponents,
                                                                          long* stats4);
        [DllImport(Lib)] public static extern int sdfk_trimesh_components_device(IntPtr trimesh, IntPtr vertexComponentDev, IntPtr triangleComponentDev,
                                                                                 long* nComponents, long* stats4);
        [DllImport(Lib)] public static extern int sdfk_trimesh_topology(IntPtr trimesh, long* census8, long* componentRows, long capacity);
        [DllImport(Lib)] public static extern int sdfk_trimesh_topology_device(IntPtr trimesh, long* census8, IntPtr componentRowsDev, long capacity);
        [DllImport(Lib)] public static extern int sdfk_trimesh_select(IntPtr trimesh, byte* keepComponent, int* vertexIndexOut, int* triangleIndexOut,
                                                                      int* trianglesOut, float* verticesOut, float* colorsOut, long* nvOut, long* ntOut);
        [DllImport(Lib)] public static extern int sdfk_trimesh_select_device(IntPtr trimesh, IntPtr keepComponentDev, IntPtr vertexIndexOutDev,
                                                                             IntPtr triangleIndexOutDev, IntPtr trianglesOutDev, IntPtr verticesOutDev,
                                                                             IntPtr colorsOutDev, long* nvOut, long* ntOut);
        [DllImport(Lib)] public static extern int sdfk_trimesh_adjacency(IntPtr trimesh, uint* nbrStart, uint* nbr, byte* boundary, long* nEntries);
        [DllImport(Lib)] public static extern int sdfk_trimesh_adjacency_device(IntPtr trimesh, IntPtr nbrStartDev, IntPtr nbrDev, IntPtr boundaryDev,
                                                                                long* nEntries);
        [DllImport(Lib)] public static extern int sdfk_trimesh_smooth(IntPtr trimesh, int iterations, float lambda, float mu, int flags, float* vertices3Out);
        [DllImport(Lib)] public static extern int sdfk_trimesh_smooth_device(IntPtr trimesh, int iterations, float lambda, float mu, int flags,
                                                                             IntPtr vertices3OutDev);
        [DllImport(Lib)] public static extern int sdfk_trimesh_vertex_normals(IntPtr trimesh, float* positions3, int flags, float* normals3Out);
        [DllImport(Lib)] public static extern int sdfk_trimesh_vertex_normals_device(IntPtr trimesh, IntPtr positions3Dev, int flags, IntPtr normals3OutDev);
        [DllImport(Lib)] public static extern int sdfk_trimesh_weld(IntPtr trimesh, float tolerance, int flags, int* vertexMap, int* vertexIndexOut,
                                                                    int* triangleIndexOut, int* trianglesOut, float* verticesOut, float* colorsOut,
                                                                    long* nvOut, long* ntOut, long* stats4);
        [DllImport(Lib)] public static extern int sdfk_trimesh_weld_device(IntPtr trimesh, float tolerance, int flags, IntPtr vertexMapDev,
                                                                           IntPtr vertexIndexOutDev, IntPtr triangleIndexOutDev, IntPtr trianglesOutDev,
                                                                           IntPtr verticesOutDev, IntPtr colorsOutDev, long* nvOut, long* ntOut, long* stats4);
        [DllImport(Lib)] public static extern int sdfk_trimesh_simplify(IntPtr trimesh, float cellSize, int placement, int flags, int* vertexMap,
                                                                        int* vertexIndexOut, int* triangleIndexOut, int* trianglesOut, float* verticesOut,
                                                                        float* colorsOut, long* nvOut, long* ntOut, long* stats6);
        [DllImport(Lib)] public static extern int sdfk_trimesh_simplify_device(IntPtr trimesh, float cellSize, int placement, int flags, IntPtr vertexMapDev,
                                                                               IntPtr vertexIndexOutDev, IntPtr triangleIndexOutDev, IntPtr trianglesOutDev,
                                                                               IntPtr verticesOutDev, IntPtr colorsOutDev, long* nvOut, long* ntOut, long* stats6);
        [DllImport(Lib)] public static extern int sdfk_trimesh_raycast(IntPtr trimesh, float* origins3, float* directions3, long n, float tMin, float tMax,
                                                                       int flags, int* triangle, float* distance, float* weights3);
        [DllImport(Lib)] public static extern int sdfk_trimesh_raycast_device(IntPtr trimesh, IntPtr origins3Dev, IntPtr directions3Dev, long n, float tMin,
                                                                              float tMax, int flags, IntPtr triangleDev, IntPtr distanceDev, IntPtr weights3Dev);
        [DllImport(Lib)] public static extern int sdfk_trimesh_render(IntPtr trimesh, int width, int height, float* cameraPosition, float* viewProjectionInverse,
                                                                      float near, float far, float* depth, float* rgb, int* triangle);
        [DllImport(Lib)] public static extern int sdfk_trimesh_render_device(IntPtr trimesh, int width, int height, float* cameraPosition,
                                                                             float* viewProjectionInverse, float near, float far, IntPtr depthDev, IntPtr rgbDev,
                                                                             IntPtr triangleDev);
        [DllImport(Lib)] public static extern int sdfk_trimesh_winding(IntPtr trimesh, float* queries3, long n, float beta, float* winding, byte* inside);
        [DllImport(Lib)] public static extern int sdfk_trimesh_winding_device(IntPtr trimesh, IntPtr queries3Dev, long n, float beta, IntPtr windingDev,
                                                                              IntPtr insideDev);
        [DllImport(Lib)] public static extern int sdfk_trimesh_to_volume_signed(IntPtr trimesh, IntPtr volume, float maxDistance, int signMode, float beta);
        [DllImport(Lib)] public static extern int sdfk_trimesh_winding_stats(IntPtr trimesh, long* stats8);
        [DllImport(Lib)] public static extern void sdfk_trimesh_free(IntPtr trimesh);
        [DllImport(Lib)] public static extern int sdfk_volume_redistance(IntPtr src, IntPtr dst, float isoValue, float maxDistance, long* stats4);
        [DllImport(Lib)] public static extern int sdfk_volume_integrate_depth(IntPtr values, IntPtr weights, float* depth, int width, int height,
                                                                              float* cameraPosition, float* viewProjection, SdfkFusionParams* prm, long* stats4);
        [DllImport(Lib)] public static extern int sdfk_volume_integrate_depth_device(IntPtr values, IntPtr weights, IntPtr depthDev, int width, int height,
                                                                                     float* cameraPosition, float* viewProjection, SdfkFusionParams* prm,
                                                                                     long* stats4);
        [DllImport(Lib)] public static extern int sdfk_depth_unproject(float* depth, float* rgb, int width, int height, float* cameraPosition,
                                                                       float* viewProjectionInverse, float depthMin, float depthMax, float* points3,
                                                                       float* colors3, int* pixel, out long nValid);
        [DllImport(Lib)] public static extern int sdfk_depth_unproject_device(IntPtr depthDev, IntPtr rgbDev, int width, int height, float* cameraPosition,
                                                                              float* viewProjectionInverse, float depthMin, float depthMax, IntPtr points3Dev,
                                                                              IntPtr colors3Dev, IntPtr pixelDev, out long nValid);
        // several GPUs from ONE process (the managed host is one process): include/sdfkit_hip.h, "one process, several GPUs"
        [DllImport(Lib)] public static extern int sdfk_node_open(int* devices, int nDevices, out IntPtr node);
        [DllImport(Lib)] public static extern int sdfk_node_info(IntPtr node, out int world, out int backend);
        [DllImport(Lib)] public static extern int sdfk_node_to_mesh(IntPtr node, SdfkOp* ops, int nOps, int* outRgbw, int writesColor, float* min, float* max,
                                                                    int nx, int ny, int nz, int clip, float iso, out IntPtr mesh);
        [DllImport(Lib)] public static extern int sdfk_node_mesh_begin(IntPtr node, SdfkOp* ops, int nOps, int* outRgbw, int writesColor, float* min, float* max,
                                                                       int nx, int ny, int nz, int clip, float iso, out long nVertices, out long nIndices, out int hasColors);
        [DllImport(Lib)] public static extern int sdfk_node_mesh_copy(IntPtr node, float* vertices3, float* colors3, float* normals3, int* triangles, float* min, float* max);
        [DllImport(Lib)] public static extern void sdfk_node_close(IntPtr node);
        // RayMarcher (RayMarcher.cs:45-211)
        [DllImport(Lib)] public static extern int sdfk_raymarch(IntPtr program, int width, int height, float* cameraPosition, float* viewProjectionInverse,
                                                                float near, float far, int depthIterations, float* depth, float* rgb);

        static readonly object initLock = new object();
        static bool inited;

        /// <summary>enum sdfk_option</summary>
        public const int OptLanes = 1, OptTokens = 2, OptGraphs = 3, OptCopyMode = 4, OptCornerEval = 5, OptVcolorEval = 6,
                         OptDistExchange = 7, OptDistLanes = 8, OptHwQueues = 9, OptCodeCache = 10, OptPrefaultHuge = 11, OptDistIndex16 = 12, OptStreamPlacement = 13, OptIdleLane = 14, OptIdlePrograms = 15, OptElideVolume = 16, OptColorPasses = 17;

        /// <summary>sdfk_init once per process; device = LOCAL_RANK (one process per GPU) or 0.</summary>
        public static void EnsureInit()
        {
            if (inited) return;
            lock (initLock) {
                if (inited) return;
                // (the entry points this shim binds -- sdfk_set_option, sdfk_dist_*, sdfk_mesh_size_hint -- are ABI 4; ABI 5 changed a default)
                if (sdfk_abi_version() != 6) throw new InvalidOperationException("libsdfkit_hip.so does not have the ABI version (6) this shim was written for");
                int device = int.TryParse(Environment.GetEnvironmentVariable("LOCAL_RANK"), out var r) ? r : 0;
                Check(sdfk_init(device));
                inited = true;
            }
        }

        /// <summary>The reference throws nothing on this path; a native failure becomes InvalidOperationException.</summary>
        public static void Check(int status)
        {
            if (status != 0)
                throw new InvalidOperationException($"sdfkit_hip status {status}: {Marshal.PtrToStringAnsi(sdfk_last_error())}");
        }
    }
}
