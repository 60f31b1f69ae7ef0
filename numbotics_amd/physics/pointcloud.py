"""Point-cloud obstacles: N points of one radius in a uniform grid on the device (include/nbk.h, nbk_cloud_*).

A ``PointCloud`` belongs to no robot: ``Arm.in_collision_with_cloud`` / ``Arm.cloud_clearance`` and
``DeviceModel.cloud_validity`` / ``cloud_clearance`` take it as an argument, and one cloud serves many arms.  ``update`` swaps the
points in place on the current stream (no allocation, no synchronisation, capturable), so a depth camera's frames cost one update
each and never a new descriptor.  Like the rest of the device path it has no CPU form.
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

    def update(self, points, radius=None):
        """Replace the points (and, optionally, the radius) on the current stream: nbk_cloud_set_points.  A CUDA tensor is read in
        place when the update runs -- keep it unchanged until then (the cloud holds a reference to the last one)."""
        import torch
        t = self._device_points(torch, points)
        n = int(t.shape[0])              # (more than `capacity` points: the library refuses the update, NBK_ERR_INVALID)
        radius = self.radius if radius is None else float(radius)
        if not radius >= 0.0:
            raise ValueError(f"radius must be >= 0, got {radius}")
        _lib.check(self._lib.nbk_cloud_set_points(self._h, t.data_ptr() if n > 0 else None, n, radius,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nbk_cloud_set_points")
        self.radius = radius             # (only now: a refused update leaves the object as the device has it)
        self._points = t
        self.n = n

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
