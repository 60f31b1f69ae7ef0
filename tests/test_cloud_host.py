"""Point-cloud obstacles, the part that needs no device: the argument rules of nbk_cloud_create (answered before any device is looked
for), the cell rule of nbk_cloud_cells_host against a NumPy restatement, and the header / binding agreement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
CLOUD_SYMBOLS = {"nbk_cloud_create", "nbk_cloud_destroy", "nbk_cloud_set_points", "nbk_cloud_status", "nbk_cloud_validity_batch",
                 "nbk_cloud_clearance_batch", "nbk_cloud_cells_host"}


def _create(lib, capacity, lo, cell, dims, out=True):
    lo_a = None if lo is None else np.asarray(lo, dtype=np.float64)
    dims_a = None if dims is None else np.asarray(dims, dtype=np.int32)
    h = C.c_void_p()
    rc = lib.nbk_cloud_create(capacity, None if lo_a is None else lo_a.ctypes.data, cell, None if dims_a is None else dims_a.ctypes.data,
                              C.byref(h) if out else None)
    return rc, h


BAD = {
    "null lo": (10, None, 0.1, (4, 4, 4)),
    "null dims": (10, (0, 0, 0), 0.1, None),
    "capacity 0": (0, (0, 0, 0), 0.1, (4, 4, 4)),
    "capacity negative": (-5, (0, 0, 0), 0.1, (4, 4, 4)),
    "capacity above 2^24": ((1 << 24) + 1, (0, 0, 0), 0.1, (4, 4, 4)),
    "cell NaN": (10, (0, 0, 0), float("nan"), (4, 4, 4)),
    "cell 0": (10, (0, 0, 0), 0.0, (4, 4, 4)),
    "cell negative": (10, (0, 0, 0), -0.1, (4, 4, 4)),
    "lo NaN": (10, (0, float("nan"), 0), 0.1, (4, 4, 4)),
    "lo infinite": (10, (0, 0, float("-inf")), 0.1, (4, 4, 4)),
    "dim 0": (10, (0, 0, 0), 0.1, (4, 0, 4)),
    "dim negative": (10, (0, 0, 0), 0.1, (-1, 4, 4)),
    "more than 2^22 cells": (10, (0, 0, 0), 0.1, (256, 256, 65)),
    "product overflows int32": (10, (0, 0, 0), 0.1, (65536, 65536, 4)),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_cloud_create_refuses_bad_arguments_before_any_device(case):
    from numbotics_amd import _lib
    lib = _lib.load()
    rc, h = _create(lib, *BAD[case])
    assert rc == INVALID, (case, rc)
    assert not h.value


def test_cloud_create_refuses_a_null_result_pointer_and_the_rest_is_null_safe():
    from numbotics_amd import _lib
    lib = _lib.load()
    rc, _ = _create(lib, 10, (0, 0, 0), 0.1, (4, 4, 4), out=False)
    assert rc == INVALID
    lib.nbk_cloud_destroy(None)
    st = C.c_int32(7)
    assert lib.nbk_cloud_status(None, C.byref(st)) == INVALID
    assert lib.nbk_cloud_set_points(None, None, 0, 0.0, None) == INVALID
    assert lib.nbk_cloud_validity_batch(None, None, None, 0, 0.0, None, 0, None, None, None) == INVALID
    assert lib.nbk_cloud_clearance_batch(None, None, None, 0, 0.1, None, None, None, None, None) == INVALID


def _cells_numpy(lo, cell, dims, pts):
    """The cell rule restated: floor((x - lo) / cell) in float64, clamped to [0, dim - 1]; x fastest."""
    c = np.floor((pts - lo[None, :]) / cell)
    c = np.clip(c, 0, (dims - 1)[None, :]).astype(np.int64)
    return ((c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]).astype(np.int32)


@pytest.mark.parametrize("cell", [1e-3, 0.05, 0.37, 10.0, 1e3])
def test_cloud_cells_host_equals_the_numpy_rule(cell):
    from numbotics_amd.physics.pointcloud import cells_host
    rng = np.random.default_rng(11)
    dims = np.array([17, 5, 33], dtype=np.int32)
    lo = np.array([-0.3, 0.2, -1.0]) * cell * 10
    ext = dims * cell
    pts = lo[None, :] + rng.uniform(-0.3, 1.3, (10000, 3)) * ext[None, :]      # a third of them outside the box: clamped
    # exact multiples of the cell from lo, the box's corners and far away points
    k = rng.integers(-2, 36, (500, 3))
    pts[:500] = lo[None, :] + k * cell
    pts[500] = lo; pts[501] = lo + ext; pts[502] = [1e300, -1e300, 0.0]; pts[503] = [np.inf, -np.inf, 0.0]
    got = cells_host(lo, cell, dims, pts)
    want = _cells_numpy(lo, cell, dims.astype(np.int64), pts)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert 0 <= got.min() and got.max() < int(np.prod(dims))
    assert len(np.unique(got)) > 100
    # a NaN coordinate has cell coordinate 0 on its axis (the device raises the cloud's status for such a point)
    nan_pt = np.array([[np.nan, lo[1] + 2.5 * cell, lo[2] + 1.5 * cell]])
    assert cells_host(lo, cell, dims, nan_pt)[0] == (1 * 5 + 2) * 17 + 0


def test_cloud_cells_host_argument_errors():
    from numbotics_amd import _lib
    lib = _lib.load()
    lo = np.zeros(3); dims = np.array([4, 4, 4], dtype=np.int32); pts = np.zeros((2, 3)); out = np.zeros(2, dtype=np.int32)
    assert lib.nbk_cloud_cells_host(lo.ctypes.data, 0.1, dims.ctypes.data, pts.ctypes.data, 2, out.ctypes.data) == 0
    assert lib.nbk_cloud_cells_host(lo.ctypes.data, 0.1, dims.ctypes.data, None, 0, None) == 0
    assert lib.nbk_cloud_cells_host(lo.ctypes.data, 0.0, dims.ctypes.data, pts.ctypes.data, 2, out.ctypes.data) == INVALID
    assert lib.nbk_cloud_cells_host(lo.ctypes.data, 0.1, dims.ctypes.data, None, 2, out.ctypes.data) == INVALID
    assert lib.nbk_cloud_cells_host(lo.ctypes.data, 0.1, dims.ctypes.data, pts.ctypes.data, -1, out.ctypes.data) == INVALID


def test_cloud_symbols_are_declared_bound_and_exported():
    from numbotics_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "nbk.h")).read()
    declared = {s for s in re.findall(r"\b(nbk_[a-z_]+)\s*\(", header) if s.startswith("nbk_cloud_")}
    assert declared == CLOUD_SYMBOLS
    assert CLOUD_SYMBOLS <= set(_lib.SYMBOLS)
    for s in CLOUD_SYMBOLS:
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    assert "#define NBK_ABI_VERSION 2" in header


def test_default_grid_fits_the_cell_limit():
    from numbotics_amd.physics.pointcloud import default_grid, MAX_CELLS
    cell, dims = default_grid([0, 0, 0], [1.21, 1.21, 1.01], 0.05)
    assert cell == 0.05 and tuple(dims) == (25, 25, 21)
    cell, dims = default_grid([0, 0, 0], [100.0, 100.0, 50.0], 0.05)
    assert cell > 0.05 and int(np.prod(dims.astype(np.int64))) <= MAX_CELLS
    cell, dims = default_grid([1, 1, 1], [1, 1, 1], 0.05)
    assert tuple(dims) == (1, 1, 1)
