"""Point-cloud obstacles: N points of one radius in a uniform grid on the device (include/nbk.h, nbk_cloud_*).

A ``PointCloud`` belongs to no robot: ``Arm.in_collision_with_cloud`` / ``Arm.cloud_clearance`` and
``DeviceModel.cloud_validity`` / ``cloud_clearance`` take it as an argument, and one cloud serves many arms.  ``update`` swaps the
points in place on the current stream (no allocation, no synchronisation, capturable), so a depth camera's frames cost one update
each and never a new descriptor.  Like the rest of the device path it has no CPU form.

From a camera's frame to that update: ``backproject`` (a depth image to world points and a validity mask, one pixel per point),
``Arm.cloud_self_filter`` (the arm's own image out of the mask) and ``update(points, keep=mask)``; ``update_from_depth`` is the
three on the current stream.
"""
import ctypes as C

import numpy as np

from numbotics_amd import _lib

MAX_CELLS = 1 << 22
MAX_POINTS = 1 << 24
# Default cell size: max(DEFAULT_CELL, 2 * radius), enlarged until the grid has at most MAX_CELLS cells.  The query of one robot shape
# walks the cells of a ball of about (bounding radius of the link + threshold + radius): cells much smaller than that ball cost row
# look-ups and a longer scan in every update, cells much larger cost bounding-sphere tests on points that cannot touch.  0.03 is the
# cell the sweep of tools/cloud_time.py supports (c2, 1e5 points, 1e5 configurations: validity 10.9 ms at 0.03, 11.2 at 0.02, 13.7 at
# 0.05, 24.4 at 0.1; the update 0.16 ms at 0.03 and 2.0 ms at 0.0125; profiles/cloud_time.log).
DEFAULT_CELL = 0.03


def default_grid(lo, hi, cell):
    """(cell, dims) of a grid over the box [lo, hi]: ``cell`` enlarged (x 1.25 a step) until the grid fits MAX_CELLS cells."""
    ext = np.maximum(np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64), 0.0)
    cell = float(cell)
    while True:
        dims = np.maximum(np.floor(ext / cell).astype(np.int64) + 1, 1)
        if int(dims[0]) * int(dims[1]) * int(dims[2]) <= MAX_CELLS:
            return cell, dims.astype(np.int32)
        cell *= 1.25


def cells_host(lo, cell, dims, points):
    """Cell index of each point by the library's own routine on the host (nbk_cloud_cells_host; no GPU needed)."""
    lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(3)
    dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(3)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    out = np.empty((pts.shape[0],), dtype=np.int32)
    _lib.check(_lib.load().nbk_cloud_cells_host(lo.ctypes.data, float(cell), dims.ctypes.data, pts.ctypes.data, pts.shape[0],
                                                out.ctypes.data), "nbk_cloud_cells_host")
    return out


def intrinsics_from_fov(width, height, fov_deg):
    """(fx, fy, cx, cy) of a ``width`` x ``height`` image with the vertical field of view ``fov_deg``: ``fy = (height / 2) /
    tan(fov / 2)``, ``fx = fy`` (square pixels: the projection of ``World.depth_image``, whose aspect is width / height),
    ``cx = (width - 1) / 2``, ``cy = (height - 1) / 2`` -- the rays go through the pixel centres."""
    fy = (float(height) / 2.0) / np.tan(np.deg2rad(float(fov_deg)) / 2.0)
    return float(fy), float(fy), (float(width) - 1.0) / 2.0, (float(height) - 1.0) / 2.0


def _intrinsics(intrinsics):
    """(fx, fy, cx, cy) from that tuple or from a 3 x 3 camera matrix."""
    k = np.asarray(intrinsics, dtype=np.float64)
    if k.shape == (3, 3):
        return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
    if k.shape != (4,):
        raise ValueError(f"intrinsics must be (fx, fy, cx, cy) or a 3 x 3 matrix, got shape {k.shape}")
    return float(k[0]), float(k[1]), float(k[2]), float(k[3])


def optical_pose(camera_pose, frame="optical"):
    """The (3, 4) float64 pose of the camera's OPTICAL frame (z forward, x right, y down) from a NumPy (4, 4) or (3, 4) pose.
    ``frame="numbotics"``: ``camera_pose`` is the reference's camera frame (looking along x, z up): it is multiplied from the right
    by the signed permutation with the optical axes x = -y_cam, y = -z_cam, z = x_cam -- columns moved and negated, nothing rounded."""
    T = np.asarray(camera_pose, dtype=np.float64)
    if T.shape not in ((4, 4), (3, 4)):
        raise ValueError(f"camera_pose must be (4, 4) or (3, 4), got {T.shape}")
    T = T[:3, :4]
    if frame == "optical":
        return np.ascontiguousarray(T)
    if frame != "numbotics":
        raise ValueError(f"frame must be 'optical' or 'numbotics', got {frame!r}")
    return np.ascontiguousarray(np.stack((-T[:, 1], -T[:, 2], T[:, 0], T[:, 3]), axis=1))


def _depth_array(torch, depth):
    """``depth`` as a contiguous (H, W) tensor, float32 or int16 (16-bit images are read as unsigned raw units whatever their
    signedness says: int16 carries the bits); a CUDA tensor stays where it is, anything else becomes a host tensor."""
    if torch.is_tensor(depth):
        t = depth
        if t.dtype not in (torch.float32, torch.int16):
            if t.dtype == getattr(torch, "uint16", None):
                t = t.view(torch.int16)
            else:
                raise ValueError(f"depth must be float32 or 16-bit, got {t.dtype}")
    else:
        a = np.asarray(depth)
        if a.dtype in (np.uint16, np.int16):
            a = np.ascontiguousarray(a).view(np.int16)
        elif a.dtype == np.float32:
            a = np.ascontiguousarray(a)
        else:
            raise ValueError(f"depth must be float32 or 16-bit, got {a.dtype}")
        t = torch.from_numpy(a)
    if t.ndim != 2 or not t.is_contiguous():
        raise ValueError(f"depth must be a contiguous (H, W) image, got {tuple(t.shape)}")
    return t


def _device_keep(torch, keep, n):
    """``keep`` as a contiguous (n,) uint8 CUDA tensor (a bool tensor is read as it is: one byte each)."""
    if torch.is_tensor(keep):
        k = keep
        if not k.is_cuda or k.dtype not in (torch.uint8, torch.bool) or not k.is_contiguous():
            raise ValueError("keep on the device must be a contiguous uint8 / bool CUDA tensor")
        k = k.view(torch.uint8) if k.dtype == torch.bool else k
    else:
        k = torch.from_numpy(np.ascontiguousarray(np.asarray(keep).astype(bool)).view(np.uint8)).to("cuda")
    if tuple(k.shape) != (n,):
        raise ValueError(f"keep must have shape ({n},), got {tuple(k.shape)}")
    return k


def backproject_host(depth, intrinsics, camera_pose, depth_scale=1.0, z_min=0.0, z_max=np.inf, frame="optical"):
    """``backproject`` by the library's own routine on the host (nbk_frame_cloud_backproject_host; no GPU needed): NumPy in, NumPy
    (points (H * W, 3), keep (H * W,) uint8) out, the bits of the device's."""
    a = np.asarray(depth)
    if a.ndim != 2 or a.dtype not in (np.float32, np.uint16, np.int16):
        raise ValueError("depth must be a (H, W) float32 or 16-bit image")
    a = np.ascontiguousarray(a)
    fx, fy, cx, cy = _intrinsics(intrinsics)
    T = optical_pose(camera_pose, frame)
    H, W = a.shape
    pts = np.empty((H * W, 3), dtype=np.float64)
    keep = np.empty((H * W,), dtype=np.uint8)
    _lib.check(_lib.load().nbk_frame_cloud_backproject_host(a.ctypes.data, 0 if a.dtype == np.float32 else 1, H, W, float(depth_scale), fx, fy,
                                                      cx, cy, T.ctypes.data, float(z_min), float(z_max), pts.ctypes.data, keep.ctypes.data),
               "nbk_frame_cloud_backproject_host")
    return pts, keep


def backproject(depth, intrinsics, camera_pose, depth_scale=1.0, z_min=0.0, z_max=np.inf, frame="optical", out=None, _pose_stage=None):
    """A depth image to world points on the current stream (nbk_frame_cloud_backproject) -> (points (H * W, 3) float64, keep (H * W,)
    uint8), CUDA tensors; point ``v * W + u`` is pixel (u, v).  ``depth``: (H, W), NumPy or a CUDA tensor, float32 (times
    ``depth_scale``: metres) or 16-bit raw units (a torch int16 / uint16 tensor is read as unsigned bits); the metric depth along
    the view axis, as ``World.depth_image`` renders it.  ``intrinsics``: (fx, fy, cx, cy) or a 3 x 3 camera matrix
    (``intrinsics_from_fov``).  ``camera_pose``: the camera's world pose, (4, 4) or (3, 4), NumPy or a float64 CUDA tensor (read when
    the kernel runs); ``frame="optical"``: z forward, x right, y down; ``frame="numbotics"``: the reference's camera, x forward and
    z up (``optical_pose``).  A pixel counts (keep 1) iff its depth z is finite, ``z > z_min`` and ``z <= z_max``; the others --
    holes -- get keep 0 and the point (0, 0, 0).  ``out``: (points, keep) tensors to write into."""
    from numbotics_amd.engine import _require_gpu
    torch = _require_gpu()
    d = _depth_array(torch, depth)
    if not d.is_cuda:
        d = d.to("cuda")
    H, W = int(d.shape[0]), int(d.shape[1])
    fx, fy, cx, cy = _intrinsics(intrinsics)
    if torch.is_tensor(camera_pose):
        T = camera_pose
        if not T.is_cuda or T.dtype != torch.float64 or tuple(T.shape) not in ((4, 4), (3, 4)) or not T.is_contiguous():
            raise ValueError("camera_pose on the device must be a contiguous float64 (4, 4) or (3, 4) CUDA tensor")
        if frame == "numbotics":
            stage = _pose_stage if _pose_stage is not None else torch.empty((3, 4), dtype=torch.float64, device=T.device)
            torch.neg(T[:3, 1], out=stage[:, 0])
            torch.neg(T[:3, 2], out=stage[:, 1])
            stage[:, 2].copy_(T[:3, 0])
            stage[:, 3].copy_(T[:3, 3])
            T = stage
        elif frame != "optical":
            raise ValueError(f"frame must be 'optical' or 'numbotics', got {frame!r}")
    else:
        host = torch.from_numpy(optical_pose(camera_pose, frame))
        if _pose_stage is not None:
            T = _pose_stage.copy_(host)
        else:
            T = host.to("cuda")
    if out is None:
        pts = torch.empty((H * W, 3), dtype=torch.float64, device=d.device)
        keep = torch.empty((H * W,), dtype=torch.uint8, device=d.device)
    else:
        pts, keep = out
        if not (torch.is_tensor(pts) and pts.is_cuda and pts.dtype == torch.float64 and tuple(pts.shape) == (H * W, 3) and pts.is_contiguous()
                and torch.is_tensor(keep) and keep.is_cuda and keep.dtype == torch.uint8 and tuple(keep.shape) == (H * W,) and keep.is_contiguous()):
            raise ValueError(f"out must be contiguous CUDA tensors: float64 ({H * W}, 3) and uint8 ({H * W},)")
    n = H * W
    _lib.check(_lib.load().nbk_frame_cloud_backproject(d.data_ptr() if n > 0 else None, 0 if d.dtype == torch.float32 else 1, H, W,
                                                 float(depth_scale), fx, fy, cx, cy, T.data_ptr(), float(z_min), float(z_max),
                                                 pts.data_ptr() if n > 0 else None, keep.data_ptr() if n > 0 else None,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nbk_frame_cloud_backproject")
    return pts, keep


class PointCloud:
    """``points`` (N, 3) float64 -- NumPy or a CUDA tensor --, every point a sphere of ``radius`` (0: bare points).

    ``bounds`` = (lo, hi): the box the grid covers; default: the bounding box of ``points`` (one read-back, at construction only).
    Points of later updates that fall outside it are kept in the border cells: results never depend on the box, only the time
    does.  ``cell``: default ``max(DEFAULT_CELL, 2 * radius)``, enlarged until the grid fits 2^22 cells.  ``capacity``: the most
    points an update may bring (default ``max(N, 1)``)."""

    def __init__(self, points, radius, cell=None, bounds=None, capacity=None):
        from numbotics_amd.engine import _require_gpu
        torch = _require_gpu()
        radius = float(radius)
        if not radius >= 0.0:
            raise ValueError(f"radius must be >= 0, got {radius}")
        t = self._device_points(torch, points)
        n = int(t.shape[0])
        if bounds is None:
            if n == 0:
                raise ValueError("an empty first cloud needs bounds")
            lo_t, hi_t = t.min(dim=0).values, t.max(dim=0).values
            lo, hi = lo_t.cpu().numpy(), hi_t.cpu().numpy()
            if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
                raise ValueError("the first points are not finite: give bounds")
        else:
            lo = np.asarray(bounds[0], dtype=np.float64).reshape(3)
            hi = np.asarray(bounds[1], dtype=np.float64).reshape(3)
        if cell is None:
            cell, dims = default_grid(lo, hi, max(DEFAULT_CELL, 2.0 * radius))
        else:
            cell = float(cell)
            if not cell > 0.0:
                raise ValueError(f"cell must be > 0, got {cell}")
            dims = np.maximum(np.floor(np.maximum(hi - lo, 0.0) / cell).astype(np.int64) + 1, 1)
            if int(dims[0]) * int(dims[1]) * int(dims[2]) > MAX_CELLS:
                raise ValueError(f"a grid of {tuple(int(d) for d in dims)} cells exceeds 2^22: choose a larger cell")
            dims = dims.astype(np.int32)
        self.capacity = int(capacity) if capacity is not None else max(n, 1)
        if n > self.capacity:
            raise ValueError(f"{n} points exceed capacity {self.capacity}")
        self.lo = np.ascontiguousarray(lo, dtype=np.float64)
        self.cell, self.dims = float(cell), np.ascontiguousarray(dims, dtype=np.int32)
        self.radius = radius
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.nbk_cloud_create(self.capacity, self.lo.ctypes.data, self.cell, self.dims.ctypes.data, C.byref(h)),
                   "nbk_cloud_create")
        self._h = h
        self.n = 0
        self._points = None
        self.update(t)

    @staticmethod
    def _device_points(torch, points):
        if torch.is_tensor(points):
            t = points
            if not t.is_cuda or t.dtype != torch.float64:
                raise ValueError("points on the device must be a float64 CUDA tensor")
            if t.ndim != 2 or t.shape[1] != 3 or not t.is_contiguous():
                raise ValueError(f"points must be a contiguous (N, 3) tensor, got {tuple(t.shape)}")
            return t
        a = np.ascontiguousarray(np.asarray(points, dtype=np.float64)).reshape(-1, 3)
        return torch.from_numpy(a).to("cuda")

    def update(self, points, radius=None, keep=None):
        """Replace the points (and, optionally, the radius) on the current stream: nbk_cloud_set_points.  A CUDA tensor is read in
        place when the update runs -- keep it unchanged until then (the cloud holds a reference to the last one).  ``keep``: an
        optional (N,) uint8 / bool mask -- a CUDA tensor, read in place likewise, or NumPy -- of the points that take part
        (nbk_frame_cloud_set_points): the others are neither stored nor checked for finiteness, and the cloud reports the ones
        it holds under their indices in ``points``.  ``n`` is the number submitted (what ``capacity`` bounds); ``count()`` the
        number held."""
        import torch
        t = self._device_points(torch, points)
        n = int(t.shape[0])              # (more than `capacity` points: the library refuses the update, NBK_ERR_INVALID)
        radius = self.radius if radius is None else float(radius)
        if not radius >= 0.0:
            raise ValueError(f"radius must be >= 0, got {radius}")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if keep is None:
            _lib.check(self._lib.nbk_cloud_set_points(self._h, t.data_ptr() if n > 0 else None, n, radius, stream), "nbk_cloud_set_points")
        else:
            k = _device_keep(torch, keep, n)
            _lib.check(self._lib.nbk_frame_cloud_set_points(self._h, t.data_ptr() if n > 0 else None, k.data_ptr() if n > 0 else None,
                                                             n, radius, stream), "nbk_frame_cloud_set_points")
            self._keep = k
        self.radius = radius             # (only now: a refused update leaves the object as the device has it)
        self._points = t
        self.n = n

    def count(self) -> int:
        """The points the cloud holds: those of the last update that its ``keep`` let through (all of them without one).
        Synchronises, like ``status``."""
        out = C.c_int64(0)
        _lib.check(self._lib.nbk_frame_cloud_count(self._h, C.byref(out)), "nbk_frame_cloud_count")
        return int(out.value)

    def update_from_depth(self, depth, intrinsics, camera_pose, arm=None, q=None, padding=0.0, ignore_links=(), **options):
        """A depth frame to the cloud's points on the current stream, in three steps: ``backproject`` (``options``: its
        ``depth_scale``, ``z_min``, ``z_max``, ``frame``), then -- with ``arm`` and its configuration ``q`` when the frame was
        taken -- ``arm.cloud_self_filter`` at the cloud's radius and ``padding`` (``ignore_links``: links whose image stays in),
        then ``update(points, keep=keep)``.  Point i is pixel ``v * W + u``; ``in_collision_with_cloud(q, cloud, padding)`` is
        False afterwards for the links that were filtered, exactly.  H * W must not exceed ``capacity``.

        The staging tensors (points, mask, pose, q and the frame itself) are allocated once, on the first call with a given
        H * W and depth type; after that the call allocates nothing and -- given CUDA tensors for ``depth``, ``camera_pose`` and
        ``q``, which are read when the work runs -- issues no host copy, so it may be captured in a graph that is replayed with
        those tensors rewritten in place.  Returns (points, keep), the staging tensors themselves."""
        import torch
        d = _depth_array(torch, depth)
        H, W = int(d.shape[0]), int(d.shape[1])
        st = self.__dict__.get("_stage")
        if st is None or st["key"] != (H * W, d.dtype):
            st = self._stage = {"key": (H * W, d.dtype), "pts": torch.empty((H * W, 3), dtype=torch.float64, device="cuda"),
                                "keep": torch.empty((H * W,), dtype=torch.uint8, device="cuda"),
                                "pose": torch.empty((3, 4), dtype=torch.float64, device="cuda"),
                                "depth": torch.empty((H, W), dtype=d.dtype, device="cuda"), "q": None}
        if not d.is_cuda:
            st["depth"].copy_(d.reshape(H, W))
            d = st["depth"]
        pts, keep = backproject(d, intrinsics, camera_pose, out=(st["pts"], st["keep"]), _pose_stage=st["pose"], **options)
        if arm is not None:
            if q is None:
                raise ValueError("the self-filter needs the configuration q the frame was taken at")
            if not torch.is_tensor(q):
                if st["q"] is None:
                    st["q"] = torch.empty((arm.dof,), dtype=torch.float64, device="cuda")
                st["q"].copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(q, dtype=np.float64)).reshape(arm.dof)))
                q = st["q"]
            arm.cloud_self_filter(pts, q, self.radius, padding, keep=keep, ignore_links=ignore_links)
        self.update(pts, keep=keep)
        return pts, keep

    def status(self) -> int:
        """0: the last update's points were all finite; 2: one was not -- until a clean update every configuration is reported
        colliding and every clearance NaN.  Synchronises."""
        out = C.c_int32(0)
        _lib.check(self._lib.nbk_cloud_status(self._h, C.byref(out)), "nbk_cloud_status")
        return int(out.value)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._lib.nbk_cloud_destroy(h)
            except Exception:
                pass
            self._h = None
