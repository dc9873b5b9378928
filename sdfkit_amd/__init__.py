"""sdfkit_amd -- MI355X (gfx950) implementation of SdfKit's Voxels.SampleSdf ->
MarchingCubes.CreateMesh hot path behind the reference's Sdf / Voxels / Mesh API, and of its
KdTree / IterativeClosestPoint (exact nearest-point search, rigid registration), and of the way back: triangle meshes
as signed distance volumes (MeshSdf, Mesh.ToVoxels) and as point clouds (Mesh.SamplePoints), and their connectivity
(Mesh.Components, Mesh.Topology, Mesh.RemoveSmallComponents), smoothing and normals from the geometry (Mesh.Smooth,
Mesh.RecomputeNormals), the welding that gives a triangle soup its connectivity (Mesh.Weld, Mesh.Concat), and the vertex clustering that makes a
dense mesh smaller (Mesh.Simplify).

`csrc/` holds the hand-written HIP kernels and the C ABI (include/sdfkit_hip.h);
`api` mirrors the reference's public types over that ABI.  There is no CPU path.
"""
from .api import (DefaultBatchSize, MarchingCubes, Mesh, Sdf, SdfExprs, SdfFunc, SdfFuncs, Sdfs, Voxels)
from .fusion import DepthFusion, DepthToPoints
from .expr import MathF, Mod, VMax, Vec3, Vec4
from .meshsdf import MeshAdjacency, MeshComponents, MeshSamples, MeshSdf, MeshSelection, MeshSimplify, MeshTopology, MeshWeld
from .points import IterativeClosestPoint, KdTree
from .raymarch import FloatData, Matrix4x4, RayMarcher, Vec3Data

__all__ = ["DefaultBatchSize", "MarchingCubes", "Mesh", "Sdf", "SdfExprs", "SdfFunc", "SdfFuncs", "Sdfs",
           "Voxels", "MathF", "Mod", "VMax", "Vec3", "Vec4", "FloatData", "Matrix4x4", "RayMarcher", "Vec3Data",
           "KdTree", "IterativeClosestPoint", "MeshSdf", "MeshSamples", "MeshComponents", "MeshTopology",
           "MeshSelection", "MeshAdjacency", "MeshWeld", "MeshSimplify", "DepthFusion", "DepthToPoints"]
