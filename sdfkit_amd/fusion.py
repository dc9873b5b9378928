"""Depth images over the C ABI entry points sdfk_volume_integrate_depth / sdfk_depth_unproject (include/sdfkit_hip.h, "Depth
images: fusion and unprojection"; csrc/lib_fusion.hip): DepthFusion averages depth frames with poses into a volume of truncated
signed distances (Curless & Levoy 1996) that Redistance and ToMesh turn into a surface; DepthToPoints gives a frame as a point
cloud for KdTree / RegisterPoints.  A depth frame is what RayMarcher.RenderDepth and MeshSdf.RenderDepth make: the distance along
every pixel's ray, (height, width) float32, +inf where nothing was seen.
"""
import ctypes as C

import numpy as np

from . import _native as N

f32 = np.float32

FUSE_CARVE_BEYOND = 1   # SDFK_FUSE_CARVE_BEYOND
_LENS = {"verticalFieldOfViewDegrees", "nearPlaneDistance", "farPlaneDistance"}


def _m16(m):
    return (C.c_float * 16)(*[float(x) for x in np.asarray(m, f32).ravel()])


def _frame(depth):
    d = depth.Values if hasattr(depth, "Values") else depth
    d = np.ascontiguousarray(np.asarray(d, f32))
    if d.ndim != 2:
        raise ValueError("a depth image is (height, width)")
    return d


def Camera(width, height, camera=(), **lens):
    """RayMarcher's camera for an image of this size -> (position, view_projection, view_projection_inverse, near, far).  camera:
    nothing (RayMarcher's default view), (viewTransform,) or (position, target, up); lens: verticalFieldOfViewDegrees,
    nearPlaneDistance, farPlaneDistance, with RayMarcher's defaults.  view_projection is the forward matrix ViewTransform x
    projection that Integrate takes; its inverse is what the renders and DepthToPoints take."""
    from .raymarch import Matrix4x4, RayMarcher
    unknown = set(lens) - _LENS
    if unknown:
        raise TypeError(f"unknown arguments {sorted(unknown)}")
    rm = RayMarcher(width, height, None)
    if camera:
        rm.ViewTransform = np.asarray(camera[0], f32) if len(camera) == 1 else Matrix4x4.CreateLookAt(*camera)
    if lens.get("verticalFieldOfViewDegrees") is not None:
        rm.VerticalFieldOfViewDegrees = lens["verticalFieldOfViewDegrees"]
    if lens.get("nearPlaneDistance") is not None:
        rm.NearPlaneDistance = lens["nearPlaneDistance"]
    if lens.get("farPlaneDistance") is not None:
        rm.FarPlaneDistance = lens["farPlaneDistance"]
    pos, vpi = rm.camera()
    proj = Matrix4x4.CreatePerspectiveFieldOfView(f32(rm.VerticalFieldOfViewDegrees) * f32(np.pi) / f32(180.0), f32(rm.width) / f32(rm.height),
                                                  rm.NearPlaneDistance, rm.FarPlaneDistance)
    return pos, Matrix4x4.Multiply(rm.ViewTransform, proj), vpi, rm.NearPlaneDistance, rm.FarPlaneDistance


class DepthFusion:
    """DepthFusion(min, max, nx, ny, nz, truncation, unseen=None, carve=True, maxWeight=inf): a running weighted average of
    truncated signed distances over the box.  Values and Weights are two Voxels on the device; Values starts filled with `unseen`
    (None: -truncation), Weights with zero.

    The unseen convention: a voxel no frame has observed keeps `unseen`.  With the default -truncation and carve=True (a pixel that
    saw nothing within depthMax frees the space along its ray), unseen space is solid and seen-empty space is free, so a fully
    scanned object meshes watertight.  unseen=+truncation with carve=False is the classic open surface, with a spurious sheet
    one truncation behind every observed surface."""

    def __init__(self, min, max, nx, ny, nz, truncation, unseen=None, carve=True, maxWeight=float("inf")):
        from .api import Voxels
        self.Truncation, self.Carve, self.MaxWeight = float(truncation), bool(carve), float(maxWeight)
        self.Unseen = -self.Truncation if unseen is None else float(unseen)
        self.Frames = 0
        self.Values = Voxels(np.full((int(nx), int(ny), int(nz)), self.Unseen, f32), None, min, max)
        self.Weights = Voxels(np.zeros((int(nx), int(ny), int(nz)), f32), None, min, max)
        for v in (self.Values, self.Weights):
            v._sync_to_device()
            v._host_values = v._host_colors = None   # the device copy is the truth

    def _params(self, weight, depthMin, depthMax):
        return N.FusionParams(self.Truncation, float(depthMin), float(depthMax), float(weight), self.MaxWeight,
                              FUSE_CARVE_BEYOND if self.Carve else 0)

    def _handles(self):
        for v in (self.Values, self.Weights):
            v._sync_to_device()   # (host arrays the caller took and may have edited win, as everywhere)
            v._host_values = v._host_colors = None
            v._version += 1
        return self.Values._h, self.Weights._h

    @staticmethod
    def _stats(stats, st):
        if stats is not None:
            stats.update(updated=int(st[0]), surface=int(st[1]), first=int(st[2]), valid_pixels=int(st[3]))

    def Integrate(self, depth, *camera, weight=1.0, depthMin=None, depthMax=None, stats=None, **lens):
        """One frame into the average (sdfk_volume_integrate_depth: one stated function of the volumes, the frame and the
        arguments).  depth: FloatData or a (height, width) array; camera: nothing, a view transform, or position, target, up;
        lens as MeshSdf.Render takes it -- the camera the frame was rendered with.  depthMin / depthMax: the range of depths
        that are observations (default: the near and the far plane).  stats: a dict that receives updated, surface, first,
        valid_pixels."""
        d = _frame(depth)
        height, width = d.shape
        pos, vp, _, near, far = Camera(width, height, camera, **lens)
        prm = self._params(weight, near if depthMin is None else depthMin, far if depthMax is None else depthMax)
        hv, hw = self._handles()
        st = (C.c_int64 * 4)() if stats is not None else None
        N.check(N.lib().sdfk_volume_integrate_depth(hv, hw, C.c_void_p(d.ctypes.data), width, height, N.f3(pos), _m16(vp), C.byref(prm), st))
        self.Frames += 1
        self._stats(stats, st)
        return self

    def IntegrateDevice(self, depth_dev, width, height, camera_position, view_projection, depthMin, depthMax, weight=1.0, stats=None):
        """Integrate from a depth image in device memory (a raw pointer, as MeshSdf.RenderDevice fills it), queued on the library
        stream.  camera_position (3) and view_projection (4 x 4, the forward matrix) as Camera() returns them."""
        prm = self._params(weight, depthMin, depthMax)
        hv, hw = self._handles()
        st = (C.c_int64 * 4)() if stats is not None else None
        N.check(N.lib().sdfk_volume_integrate_depth_device(hv, hw, C.c_void_p(depth_dev) if depth_dev else C.c_void_p(), int(width), int(height),
                                                           N.f3(camera_position), _m16(view_projection), C.byref(prm), st))
        self.Frames += 1
        self._stats(stats, st)
        return self

    def ToVoxels(self):
        """The averaged values as they are: projective, truncated distances; unseen voxels hold `unseen`."""
        return self.Values

    def ToMesh(self, isoValue=0.0, redistance=True):
        """The surface of the fused volume.  redistance: through Voxels.Redistance first, which makes distances of the
        projective, clamped values (the zero set stays where it is to first order)."""
        v = self.Values.Redistance(isoValue) if redistance else self.Values
        return v.ToMesh(isoValue)


def DepthToPoints(depth, *camera, rgb=None, depthMin=None, depthMax=None, **lens):
    """A depth frame as points (sdfk_depth_unproject) -> (points (n, 3) float32, colors (n, 3) float32 or None, pixels (n,) int32):
    camera + ray * depth for every pixel with depthMin <= depth <= depthMax (default: the near and the far plane), in pixel
    order; for a frame MeshSdf.RenderDepth made, that render's hit points bit for bit.  rgb: Vec3Data or (height, width, 3), the
    colours to gather.  pixels: j * width + i of every point."""
    d = _frame(depth)
    height, width = d.shape
    pos, _, vpi, near, far = Camera(width, height, camera, **lens)
    c = None
    if rgb is not None:
        c = np.ascontiguousarray(np.asarray(rgb.Values if hasattr(rgb, "Values") else rgb, f32))
        if c.shape != (height, width, 3):
            raise ValueError(f"rgb is {c.shape}, the depth image is {d.shape}")
    n = width * height
    pts, pix = np.empty((n, 3), f32), np.empty(n, np.int32)
    cols = np.empty((n, 3), f32) if c is not None else None
    k = C.c_int64()
    N.init()
    N.check(N.lib().sdfk_depth_unproject(C.c_void_p(d.ctypes.data), C.c_void_p(c.ctypes.data) if c is not None else C.c_void_p(), width, height,
                                         N.f3(pos), _m16(vpi), C.c_float(near if depthMin is None else depthMin),
                                         C.c_float(far if depthMax is None else depthMax), C.c_void_p(pts.ctypes.data),
                                         C.c_void_p(cols.ctypes.data) if cols is not None else C.c_void_p(), C.c_void_p(pix.ctypes.data), C.byref(k)))
    k = k.value
    return pts[:k].copy(), cols[:k].copy() if cols is not None else None, pix[:k].copy()
