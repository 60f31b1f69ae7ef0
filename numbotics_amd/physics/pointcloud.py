"""Point-cloud obstacles: N points of one radius in a uniform grid on the device (include/nbk.h, nbk_cloud_*).

A ``PointCloud`` belongs to no robot: ``Arm.in_collision_with_cloud`` / ``Arm.cloud_clearance`` and
``DeviceModel.cloud_validity`` / ``cloud_clearance`` take it as an argument, and one cloud serves many arms.  ``update`` swaps the
points in place on the current stream (no allocation, no synchronisation, capturable), so a depth camera's frames cost one update
each and never a new descriptor.  Like the rest of the device path it has no CPU form.

From a camera's frame to that update: ``backproject`` (a depth image to world points and a validity mask, one pixel per point),
``Arm.cloud_self_filter`` (the arm's own image out of the mask) and ``update(points, keep=mask)``; ``update_from_depth`` is the
three on the current stream.

Several frames in one cloud: ``PointCloud.integrate_depth`` keeps a store of ``capacity`` point slots on the device and, per frame,
releases the stored points the frame sees through (``carve``), drops the frame points the cloud holds already (``novel``), moves the
rest into free slots (``append``) and updates the cloud from the store -- a point's index in a record is its slot.
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


def _device_points(torch, points):
    """``points`` as a contiguous (N, 3) float64 CUDA tensor: one on the device as it is, anything else by one copy."""
    if torch.is_tensor(points):
        t = points
        if not t.is_cuda or t.dtype != torch.float64:
            raise ValueError("points on the device must be a float64 CUDA tensor")
        if t.ndim != 2 or t.shape[1] != 3 or not t.is_contiguous():
            raise ValueError(f"points must be a contiguous (N, 3) tensor, got {tuple(t.shape)}")
        return t
    a = np.ascontiguousarray(np.asarray(points, dtype=np.float64)).reshape(-1, 3)
    return torch.from_numpy(a).to("cuda")


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


def _device_pose(torch, camera_pose, frame, stage=None):
    """The optical pose as a float64 CUDA tensor the kernels read rows 0 .. 2 of: a device ``camera_pose`` in the optical frame as it
    is, anything else through ``stage`` (a (3, 4) float64 CUDA tensor; a new one when there is none) -- a device pose in the
    reference's frame by device copies, a host pose by ``optical_pose`` and one copy."""
    if torch.is_tensor(camera_pose):
        T = camera_pose
        if not T.is_cuda or T.dtype != torch.float64 or tuple(T.shape) not in ((4, 4), (3, 4)) or not T.is_contiguous():
            raise ValueError("camera_pose on the device must be a contiguous float64 (4, 4) or (3, 4) CUDA tensor")
        if frame == "numbotics":
            stage = stage if stage is not None else torch.empty((3, 4), dtype=torch.float64, device=T.device)
            torch.neg(T[:3, 1], out=stage[:, 0])
            torch.neg(T[:3, 2], out=stage[:, 1])
            stage[:, 2].copy_(T[:3, 0])
            stage[:, 3].copy_(T[:3, 3])
            T = stage
        elif frame != "optical":
            raise ValueError(f"frame must be 'optical' or 'numbotics', got {frame!r}")
    else:
        host = torch.from_numpy(optical_pose(camera_pose, frame))
        T = host.to("cuda") if stage is None else stage.copy_(host)
    return T


def _device_poses(torch, camera_pose, frame):
    """One pose by ``_device_pose``, or a batch (B, 4, 4) / (B, 3, 4) as a contiguous float64 (B, 3, 4) CUDA tensor of optical poses
    (``DeviceModel.render_depth``): a device batch of optical (B, 3, 4) poses as it is, anything else by one copy."""
    nd = camera_pose.ndim if torch.is_tensor(camera_pose) else np.asarray(camera_pose).ndim
    if nd != 3:
        return _device_pose(torch, camera_pose, frame)
    if not torch.is_tensor(camera_pose):
        a = np.asarray(camera_pose, dtype=np.float64)
        host = np.stack([optical_pose(p, frame) for p in a]) if a.shape[0] > 0 else np.zeros((0, 3, 4))
        return torch.from_numpy(np.ascontiguousarray(host)).to("cuda")
    T = camera_pose
    if not T.is_cuda or T.dtype != torch.float64 or tuple(T.shape[1:]) not in ((4, 4), (3, 4)):
        raise ValueError("camera poses on the device must be a float64 (B, 4, 4) or (B, 3, 4) CUDA tensor")
    T = T[:, :3, :]
    if frame == "numbotics":
        return torch.stack((-T[:, :, 1], -T[:, :, 2], T[:, :, 0], T[:, :, 3]), dim=2).contiguous()
    if frame != "optical":
        raise ValueError(f"frame must be 'optical' or 'numbotics', got {frame!r}")
    return T.contiguous()


class _Frame:
    """One depth frame as every nbk_frame_cloud_* image entry takes it, built once per call: ``depth`` by ``_depth_array`` (the one depth
    rule), ``H``, ``W``, ``pose`` (the optical pose) and ``args``, the twelve arguments those entries start with: depth, depth_type
    (0: float32, 1: 16 bits), H, W, depth_scale, fx, fy, cx, cy, T, z_min, z_max.  ``device=False``, for the host entries: the image
    stays in host memory, the pose is ``optical_pose``'s.  Else a host image goes to the device -- through ``stage.depth`` when a
    ``_FrameStage`` is given, which is fitted to the frame first -- and the pose is ``_device_pose``'s (through ``stage.pose``)."""

    __slots__ = ("depth", "H", "W", "pose", "args")

    def __init__(self, torch, depth, intrinsics, camera_pose, depth_scale, z_min, z_max, frame, device=True, stage=None):
        d = _depth_array(torch, depth)
        self.H, self.W = H, W = int(d.shape[0]), int(d.shape[1])
        fx, fy, cx, cy = _intrinsics(intrinsics)
        if not device:
            T = torch.from_numpy(optical_pose(camera_pose, frame))
        else:
            if stage is not None:
                stage.fit(torch, H, W, d.dtype)
            if not d.is_cuda:
                d = d.to("cuda") if stage is None else stage.depth.copy_(d)
            T = _device_pose(torch, camera_pose, frame, None if stage is None else stage.pose)
        self.depth, self.pose = d, T
        self.args = (d.data_ptr() if H * W > 0 else None, 0 if d.dtype == torch.float32 else 1, H, W, float(depth_scale), fx, fy, cx, cy,
                     T.data_ptr(), float(z_min), float(z_max))


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def backproject_host(depth, intrinsics, camera_pose, depth_scale=1.0, z_min=0.0, z_max=np.inf, frame="optical"):
    """``backproject`` by the library's own routine on the host (nbk_frame_cloud_backproject_host; no GPU needed): NumPy in, NumPy
    (points (H * W, 3), keep (H * W,) uint8) out, the bits of the device's."""
    import torch
    f = _Frame(torch, depth, intrinsics, camera_pose, depth_scale, z_min, z_max, frame, device=False)
    pts = np.empty((f.H * f.W, 3), dtype=np.float64)
    keep = np.empty((f.H * f.W,), dtype=np.uint8)
    _lib.check(_lib.load().nbk_frame_cloud_backproject_host(*f.args, pts.ctypes.data, keep.ctypes.data), "nbk_frame_cloud_backproject_host")
    return pts, keep


def ray_spans_host(height, width, intrinsics, camera_pose, centres, radii, near=0.01, far=1000.0, frame="optical"):
    """Per pixel and ball the depths at which the pixel's ray is inside the ball, clipped to [near, far], by the routine the renderer
    takes its candidates with (nbk_render_ray_spans_host; no GPU needed) -> (span (H * W, S, 2) float64, hit (H * W, S) bool); a
    ray that misses a ball has span (0, 0)."""
    fx, fy, cx, cy = _intrinsics(intrinsics)
    T = optical_pose(camera_pose, frame)
    c = np.ascontiguousarray(np.asarray(centres, dtype=np.float64)).reshape(-1, 3)
    r = np.ascontiguousarray(np.asarray(radii, dtype=np.float64)).reshape(-1)
    if r.shape[0] != c.shape[0]:
        raise ValueError(f"{c.shape[0]} centres but {r.shape[0]} radii")
    H, W, S = int(height), int(width), int(c.shape[0])
    span = np.zeros((max(H, 0) * max(W, 0), S, 2), dtype=np.float64)
    hit = np.zeros((max(H, 0) * max(W, 0), S), dtype=np.uint8)
    _lib.check(_lib.load().nbk_render_ray_spans_host(H, W, fx, fy, cx, cy, T.ctypes.data, c.ctypes.data, r.ctypes.data, S, float(near),
                                                     float(far), span.ctypes.data, hit.ctypes.data), "nbk_render_ray_spans_host")
    return span, hit.astype(bool)


def _backproject(torch, f, pts, keep):
    n = f.H * f.W
    _lib.check(_lib.load().nbk_frame_cloud_backproject(*f.args, pts.data_ptr() if n > 0 else None, keep.data_ptr() if n > 0 else None,
                                                       _stream(torch)), "nbk_frame_cloud_backproject")
    return pts, keep


def backproject(depth, intrinsics, camera_pose, depth_scale=1.0, z_min=0.0, z_max=np.inf, frame="optical", out=None):
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
    f = _Frame(torch, depth, intrinsics, camera_pose, depth_scale, z_min, z_max, frame)
    n = f.H * f.W
    if out is None:
        pts = torch.empty((n, 3), dtype=torch.float64, device=f.depth.device)
        keep = torch.empty((n,), dtype=torch.uint8, device=f.depth.device)
    else:
        pts, keep = out
        if not (torch.is_tensor(pts) and pts.is_cuda and pts.dtype == torch.float64 and tuple(pts.shape) == (n, 3) and pts.is_contiguous()
                and torch.is_tensor(keep) and keep.is_cuda and keep.dtype == torch.uint8 and tuple(keep.shape) == (n,) and keep.is_contiguous()):
            raise ValueError(f"out must be contiguous CUDA tensors: float64 ({n}, 3) and uint8 ({n},)")
    return _backproject(torch, f, pts, keep)


def carve_host(points, keep, depth, intrinsics, camera_pose, margin, window=1, depth_scale=1.0, z_min=0.0, z_max=np.inf, frame="optical"):
    """``carve`` by the library's own routine on the host (nbk_frame_cloud_carve_host; no GPU needed): NumPy in, the new mask (M,)
    uint8 out (``keep`` itself is not modified), the bits of the device's."""
    import torch
    f = _Frame(torch, depth, intrinsics, camera_pose, depth_scale, z_min, z_max, frame, device=False)
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64)).reshape(-1, 3)
    out = np.ascontiguousarray(np.asarray(keep)).astype(np.uint8)
    M = pts.shape[0]
    if out.shape != (M,):
        raise ValueError(f"keep must have shape ({M},), got {out.shape}")
    _lib.check(_lib.load().nbk_frame_cloud_carve_host(*f.args, float(margin), int(window), pts.ctypes.data, M, out.ctypes.data),
               "nbk_frame_cloud_carve_host")
    return out


def _carve(torch, f, margin, window, pts, k):
    M = int(pts.shape[0])
    _lib.check(_lib.load().nbk_frame_cloud_carve(*f.args, float(margin), int(window), pts.data_ptr() if M > 0 else None, M,
                                                 k.data_ptr() if M > 0 else None, _stream(torch)), "nbk_frame_cloud_carve")
    return k


def carve(points, keep, depth, intrinsics, camera_pose, margin, window=1, depth_scale=1.0, z_min=0.0, z_max=np.inf, frame="optical"):
    """Free-space carving on the current stream (nbk_frame_cloud_carve): a stored point the frame sees THROUGH is released.
    ``points`` (M, 3) float64 and ``keep`` (M,) uint8 -- CUDA tensors: ``keep`` is worked on in place and returned; NumPy: a new
    device mask is returned.  ``depth``, ``intrinsics``, ``camera_pose`` and the options are ``backproject``'s.  ``keep[i]`` goes to
    0 iff it was set, point i lies in front of the camera (beyond ``z_min``), its pixel and the ``window`` pixels around it on every
    side lie in the image, and every one of those (2 * window + 1)^2 pixels is a valid depth more than ``margin`` BEHIND the point.
    A hole in the window, a point behind the measured surface (occluded) or outside the image: no evidence, the point stays."""
    from numbotics_amd.engine import _require_gpu
    torch = _require_gpu()
    f = _Frame(torch, depth, intrinsics, camera_pose, depth_scale, z_min, z_max, frame)
    pts = _device_points(torch, points)
    return _carve(torch, f, margin, window, pts, _device_keep(torch, keep, int(pts.shape[0])))


def append_workspace_bytes(capacity, n):
    """Bytes of workspace ``append`` needs for a store of ``capacity`` slots and ``n`` new points (no GPU needed)."""
    b = int(_lib.load().nbk_frame_cloud_append_workspace_bytes(int(capacity), int(n)))
    if b < 0:
        raise ValueError(f"a store of {capacity} slots and {n} new points: sizes out of range")
    return b


def append(store_points, store_keep, points, keep, counts=None, slot_of=None, workspace=None):
    """The kept ``points`` into the free slots of a store on the current stream (nbk_frame_cloud_append), all CUDA tensors: the k-th
    point with ``keep != 0`` goes to the k-th slot with ``store_keep == 0`` (both ascending) until either list ends.  ``counts``
    (3,) int64 receives (slots held afterwards, appended, dropped); ``slot_of`` (N,) int32, optional, the slot of each new point
    or -1.  ``workspace``: a uint8 CUDA tensor of ``append_workspace_bytes`` bytes (allocated when not given).  Deterministic: ranks
    by prefix sums, no atomics.  -> counts."""
    from numbotics_amd.engine import _require_gpu
    torch = _require_gpu()
    sp = _device_points(torch, store_points)
    M = int(sp.shape[0])
    sk = _device_keep(torch, store_keep, M)
    if not (torch.is_tensor(store_keep) and store_keep.dtype == torch.uint8):
        raise ValueError("store_keep must be a uint8 CUDA tensor: it is written in place")
    p = _device_points(torch, points)
    N = int(p.shape[0])
    k = _device_keep(torch, keep, N)
    if counts is None:
        counts = torch.empty((3,), dtype=torch.int64, device="cuda")
    if workspace is None:
        workspace = torch.empty((append_workspace_bytes(M, N),), dtype=torch.uint8, device="cuda")
    if slot_of is not None and not (slot_of.is_cuda and slot_of.dtype == torch.int32 and tuple(slot_of.shape) == (N,) and slot_of.is_contiguous()):
        raise ValueError(f"slot_of must be a contiguous int32 CUDA tensor of shape ({N},)")
    if not (counts.is_cuda and counts.dtype == torch.int64 and tuple(counts.shape) == (3,) and counts.is_contiguous()):
        raise ValueError("counts must be a contiguous int64 CUDA tensor of shape (3,)")
    _lib.check(_lib.load().nbk_frame_cloud_append(sp.data_ptr(), sk.data_ptr(), M, p.data_ptr() if N > 0 else None, k.data_ptr() if N > 0 else None,
                                                  N, counts.data_ptr(), slot_of.data_ptr() if slot_of is not None and N > 0 else None,
                                                  workspace.data_ptr(), int(workspace.numel()), _stream(torch)), "nbk_frame_cloud_append")
    return counts


class _FrameStage:
    """The tensors a frame passes through on its way into a cloud: ``pts`` (H * W, 3), ``keep`` (H * W,) and ``depth`` (H, W), re-made
    when H, W or the depth type change; ``pose`` (3, 4); ``q`` (dof,), re-made when the arm's dof changes."""

    def __init__(self):
        self.key = self.pts = self.keep = self.depth = self.pose = self.q = None

    def fit(self, torch, H, W, dtype):
        if self.key != (H, W, dtype):
            self.key = (H, W, dtype)
            self.pts = torch.empty((H * W, 3), dtype=torch.float64, device="cuda")
            self.keep = torch.empty((H * W,), dtype=torch.uint8, device="cuda")
            self.depth = torch.empty((H, W), dtype=dtype, device="cuda")
            self.pose = torch.empty((3, 4), dtype=torch.float64, device="cuda")

    def device_q(self, torch, dof, q):
        """q as a device tensor: a host q goes through the stage's."""
        if q is None:
            raise ValueError("the self-filter needs the configuration q the frame was taken at")
        if torch.is_tensor(q):
            return q
        if self.q is None or self.q.shape[0] != dof:
            self.q = torch.empty((dof,), dtype=torch.float64, device="cuda")
        return self.q.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(q, dtype=np.float64)).reshape(dof)))


class _Map:
    """What ``integrate_depth`` keeps between frames: the store ``pts`` (capacity, 3) and ``keep`` (capacity,) and ``counts`` (3,),
    allocated once; the append workspace ``ws``, sized for frames of ``n`` pixels and re-made when ``n`` changes; and ``live``: the
    cloud's points are the store's."""

    def __init__(self):
        self.pts = self.keep = self.counts = self.ws = self.n = None
        self.live = False

    def end(self):
        """What a plain update and ``reset_map`` do to the map: the tensors stay, the next integration starts from an empty store."""
        self.live = False

    def fit(self, torch, capacity, n):
        if self.pts is None:
            self.pts = torch.zeros((capacity, 3), dtype=torch.float64, device="cuda")
            self.keep = torch.zeros((capacity,), dtype=torch.uint8, device="cuda")
            self.counts = torch.zeros((3,), dtype=torch.int64, device="cuda")
        if self.n != n:
            self.n, self.ws = n, torch.empty((append_workspace_bytes(capacity, n),), dtype=torch.uint8, device="cuda")
        return self


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
        t = _device_points(torch, points)
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
        self._points = self._keep = None      # the tensors of the last update: held so that they outlive the asynchronous work
        self._stage, self._map = _FrameStage(), _Map()
        self.update(t)

    def update(self, points, radius=None, keep=None):
        """Replace the points (and, optionally, the radius) on the current stream: nbk_cloud_set_points.  A CUDA tensor is read in
        place when the update runs -- keep it unchanged until then (the cloud holds a reference to the last one).  ``keep``: an
        optional (N,) uint8 / bool mask -- a CUDA tensor, read in place likewise, or NumPy -- of the points that take part
        (nbk_frame_cloud_set_points): the others are neither stored nor checked for finiteness, and the cloud reports the ones
        it holds under their indices in ``points``.  ``n`` is the number submitted (what ``capacity`` bounds); ``count()`` the
        number held."""
        import torch
        radius = self.radius if radius is None else float(radius)
        if not radius >= 0.0:
            raise ValueError(f"radius must be >= 0, got {radius}")
        t = _device_points(torch, points)
        self._set_points(torch, t, None if keep is None else _device_keep(torch, keep, int(t.shape[0])), radius)
        self._map.end()

    def _set_points(self, torch, t, k, radius):
        """The update itself, from device tensors: what ``update`` issues, and ``integrate_depth`` from its store."""
        n = int(t.shape[0])              # (more than `capacity` points: the library refuses the update, NBK_ERR_INVALID)
        if k is None:
            _lib.check(self._lib.nbk_cloud_set_points(self._h, t.data_ptr() if n > 0 else None, n, radius, _stream(torch)), "nbk_cloud_set_points")
        else:
            _lib.check(self._lib.nbk_frame_cloud_set_points(self._h, t.data_ptr() if n > 0 else None, k.data_ptr() if n > 0 else None,
                                                             n, radius, _stream(torch)), "nbk_frame_cloud_set_points")
        self.radius = radius             # (only now: a refused update leaves the object as the device has it)
        self._points, self._keep, self.n = t, k, n

    def count(self) -> int:
        """The points the cloud holds: those of the last update that its ``keep`` let through (all of them without one).
        Synchronises, like ``status``."""
        out = C.c_int64(0)
        _lib.check(self._lib.nbk_frame_cloud_count(self._h, C.byref(out)), "nbk_frame_cloud_count")
        return int(out.value)

    def _frame_points(self, torch, depth, intrinsics, camera_pose, depth_scale, z_min, z_max, frame, arm, q, padding, ignore_links):
        """The common start of ``update_from_depth`` and ``integrate_depth``: the frame's description, a host image, pose or q
        through the stage, the back-projection into the stage's tensors and, with ``arm``, its image out of the mask.
        -> (the frame on the device, points, keep, q on the device)."""
        st = self._stage
        f = _Frame(torch, depth, intrinsics, camera_pose, depth_scale, z_min, z_max, frame, stage=st)
        pts, keep = _backproject(torch, f, st.pts, st.keep)
        if arm is not None:
            q = st.device_q(torch, arm.dof, q)
            arm.cloud_self_filter(pts, q, self.radius, padding, keep=keep, ignore_links=ignore_links)
        return f, pts, keep, q

    def update_from_depth(self, depth, intrinsics, camera_pose, arm=None, q=None, padding=0.0, ignore_links=(), depth_scale=1.0, z_min=0.0,
                          z_max=np.inf, frame="optical"):
        """A depth frame to the cloud's points on the current stream, in three steps: ``backproject`` (with its ``depth_scale``,
        ``z_min``, ``z_max``, ``frame``), then -- with ``arm`` and its configuration ``q`` when the frame was
        taken -- ``arm.cloud_self_filter`` at the cloud's radius and ``padding`` (``ignore_links``: links whose image stays in),
        then ``update(points, keep=keep)``.  Point i is pixel ``v * W + u``; ``in_collision_with_cloud(q, cloud, padding)`` is
        False afterwards for the links that were filtered, exactly.  H * W must not exceed ``capacity``.

        The staging tensors (points, mask, pose, q and the frame itself) are allocated once, on the first call with a given
        H, W and depth type; after that the call allocates nothing and -- given CUDA tensors for ``depth``, ``camera_pose`` and
        ``q``, which are read when the work runs -- issues no host copy, so it may be captured in a graph that is replayed with
        those tensors rewritten in place.  Returns (points, keep), the staging tensors themselves."""
        import torch
        _, pts, keep, _ = self._frame_points(torch, depth, intrinsics, camera_pose, depth_scale, z_min, z_max, frame, arm, q, padding, ignore_links)
        self._set_points(torch, pts, keep, self.radius)
        self._map.end()
        return pts, keep

    def novel(self, points, keep, merge_distance, held=None):
        """Which of ``points`` (N, 3) the cloud does not hold yet, on the current stream (nbk_frame_cloud_novel): ``keep[i]`` goes to
        0 iff it was set and a point of the cloud lies closer than ``merge_distance`` (squared distance, strictly below the
        square).  ``held``: an optional uint8 / bool CUDA mask over the points SUBMITTED to the last update (``n`` of them): cloud
        points whose byte is 0 do not count -- a store's mask after slots were released.  ``keep`` as a CUDA tensor is worked on
        in place and returned; NumPy: a new device mask.  ``merge_distance <= 0`` drops nothing.  The cloud's size, status and grid
        are read when the work runs: an empty cloud, or one whose status is set, leaves ``keep`` as it is.  The points are not
        thinned against each other."""
        import torch
        p = _device_points(torch, points)
        n = int(p.shape[0])
        k = _device_keep(torch, keep, n)
        h = None if held is None else _device_keep(torch, held, self.n)
        _lib.check(self._lib.nbk_frame_cloud_novel(self._h, p.data_ptr() if n > 0 else None, n, float(merge_distance),
                                                   h.data_ptr() if h is not None and self.n > 0 else None, k.data_ptr() if n > 0 else None,
                                                   _stream(torch)), "nbk_frame_cloud_novel")
        return k

    def reset_map(self):
        """Forget the map: the next ``integrate_depth`` starts from an empty store.  (Issues nothing; the cloud keeps its points
        until then.)"""
        self._map.end()

    def integrate_depth(self, depth, intrinsics, camera_pose, arm=None, q=None, padding=0.0, ignore_links=(), carve_margin=0.05,
                        carve_window=1, merge_distance=None, clear_robot=True, depth_scale=1.0, z_min=0.0, z_max=np.inf, frame="optical"):
        """ADD a depth frame to the cloud, on the current stream -- where ``update_from_depth`` replaces the cloud by the frame.  The
        cloud becomes a MAP: a store of ``capacity`` point slots on the device, the cloud built from it with the masked update, so
        a point's index in every clearance or proximity record is its slot and stays that for as long as the point lives.  Seven
        steps: ``backproject`` (with its ``depth_scale``, ``z_min``, ``z_max``, ``frame``); with ``arm`` and ``q``, the
        arm's own image out of the frame (``padding``, ``ignore_links``: as ``update_from_depth``); ``carve``: stored points the
        frame sees through are released (``carve_margin``, ``carve_window``); with ``arm`` and ``clear_robot``, the stored points
        the arm now touches are released as well (the arm is where it is: no obstacle is there); ``novel``: frame points the map
        already holds within ``merge_distance`` (default: the cloud's radius, which then must not be 0) are dropped; ``append``: the
        rest moves into free slots, and what finds none is dropped and counted; then the update from the store.

        The first call, and the first after ``reset_map`` or after a plain ``update`` / ``update_from_depth`` (which end the
        map), starts from an empty store.  Store, staging and workspace are allocated once (at ``capacity`` and H * W); after that the
        call allocates nothing and, given CUDA tensors for ``depth``, ``camera_pose`` and ``q``, may be captured in a graph.  The
        frame may have fewer or more pixels than ``capacity``.  Returns (store_points (capacity, 3), store_keep (capacity,)), the
        store's own tensors; ``map_counts()`` tells what the call did.

        What carving cannot know: there is no notion of unknown space and no confidence per point -- one frame that sees through a
        point releases it --, and the world is taken to stand still while a frame is taken."""
        import torch
        merge = self.radius if merge_distance is None else float(merge_distance)
        if merge_distance is None and not merge > 0.0:
            raise ValueError("a cloud of radius 0 needs merge_distance")
        if merge != merge:
            raise ValueError("merge_distance is NaN")
        f, pts, keep, q = self._frame_points(torch, depth, intrinsics, camera_pose, depth_scale, z_min, z_max, frame, arm, q, padding, ignore_links)
        mp = self._map.fit(torch, self.capacity, f.H * f.W)
        sp, sk = mp.pts, mp.keep
        if not mp.live:
            sk.zero_()
            self._set_points(torch, sp, sk, self.radius)
            mp.live = True
        _carve(torch, f, carve_margin, carve_window, sp, sk)
        if arm is not None and clear_robot:
            arm.cloud_self_filter(sp, q, self.radius, padding, keep=sk, ignore_links=ignore_links)
        self.novel(pts, keep, merge, held=sk)
        append(sp, sk, pts, keep, counts=mp.counts, workspace=mp.ws)
        self._set_points(torch, sp, sk, self.radius)
        return sp, sk

    def map_counts(self):
        """{"held", "appended", "dropped"} of the last ``integrate_depth``: the slots held after it, the frame points it filed and
        the ones that found no free slot.  Synchronises, like ``count``."""
        if self._map.counts is None:
            raise ValueError("no frame has been integrated")
        self.count()
        held, appended, dropped = (int(x) for x in self._map.counts.cpu().numpy())
        return {"held": held, "appended": appended, "dropped": dropped}

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
