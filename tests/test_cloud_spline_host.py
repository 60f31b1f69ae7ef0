"""B-spline trajectories against a point cloud, the part that needs no device: the four entry points declared, bound and exported;
the workspace size; every argument rule of nbk_spline_cloud_validity_batch and nbk_spline_cloud_continuous_batch that is answered before
a device is looked for; the per-shape span bounds (nbk_spline_shape_motion_bounds_host) against the pair bound of the same shape with
a world shape, an independent NumPy construction and the edge's bound; and the ``cloud=`` keyword of the trajectory methods of both
connectors on a stub device (scene first, then the cloud accumulating into the scene's arrays)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from numbotics_amd.planning import unit_bspline, unit_knots
from numbotics_amd.scenes import build_scene
from cloud_cases import cloud_model
from continuous_ref import random_edges, tree_scene
from spline_ref import random_splines
from spline_continuous_ref import motion_bounds_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
nan, inf = float("nan"), float("inf")


def test_symbols_are_declared_bound_and_exported():
    from numbotics_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "nbk.h")).read()
    declared = set(re.findall(r"\b(nbk_[a-z_]+)\s*\(", header))
    for s in ("nbk_spline_cloud_workspace_bytes", "nbk_spline_cloud_validity_batch", "nbk_spline_cloud_continuous_batch",
              "nbk_spline_shape_motion_bounds_host"):
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    assert len(lib.nbk_spline_cloud_validity_batch.argtypes) == 17
    assert len(lib.nbk_spline_cloud_continuous_batch.argtypes) == 17
    assert len(lib.nbk_spline_shape_motion_bounds_host.argtypes) == 7
    assert "#define NBK_ABI_VERSION 2" in header


def test_workspace_bytes_are_linear_in_the_trajectories():
    from numbotics_amd import _lib
    from numbotics_amd.engine import DeviceModel
    size = _lib.load().nbk_spline_cloud_workspace_bytes
    assert size(0) >= 0
    sizes = [size(S) for S in (0, 1, 2, 7, 8, 9, 63, 64, 65, 1000, 10**6, 2**26 - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert size(10**6) >= 40 * 10**6, "plan (2 doubles), count, offset and first hit of every trajectory"
    assert size(10**6) <= 40 * 10**6 + 4 * 64 + 8, "... and nothing that grows with the samples: only the parts' rounding on top"
    assert size(2 * 10**6) - size(10**6) == 40 * 10**6
    for S in (-1, -2**31, -2**62):
        assert size(S) < 0
    assert DeviceModel.cloud_spline_workspace_bytes(1000) == size(1000)


# ---- the argument rules ----------------------------------------------------------------------------------------------------------
ORDER_A = ("m", "c", "ctrl", "S", "n_ctrl", "degree", "knots", "resolution", "threshold", "shape_bits", "accumulate", "valid", "t_hit",
           "n_samples", "workspace", "workspace_bytes", "stream")
ORDER_B = ("m", "c", "ctrl", "S", "n_ctrl", "degree", "knots", "threshold", "max_iter", "slack", "look_ahead", "shape_bits", "accumulate",
           "valid", "t_free", "status", "stream")


def _call(lib, which, **kw):
    """One of the two entries with arguments that pass every rule, except those given.  The descriptor and the cloud are stand-ins
    (zeroed memory, never dereferenced before the rules are through), the arrays are host memory never touched."""
    S = kw.get("S", 4)
    fake = (C.c_char * 4096)()
    mem = np.zeros((1 << 16,), dtype=np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 64
    a = dict(m=C.addressof(fake), c=C.addressof(fake), ctrl=base, S=S, n_ctrl=6, degree=3, knots=base, threshold=0.0, shape_bits=None,
             accumulate=0, valid=base, stream=None)
    if which == "a":
        a.update(resolution=0.05, t_hit=None, n_samples=None, workspace=base,
                 workspace_bytes=lib.nbk_spline_cloud_workspace_bytes(max(S, 0)))
    else:
        a.update(max_iter=64, slack=1e-6, look_ahead=0.05, t_free=base, status=base)
    if "workspace_offset" in kw:
        a["workspace"] = base + kw.pop("workspace_offset")
    a.update(kw)
    keep = (fake, mem)                                                                        # noqa: F841
    fn, order = (lib.nbk_spline_cloud_validity_batch, ORDER_A) if which == "a" else (lib.nbk_spline_cloud_continuous_batch, ORDER_B)
    return fn(*[a[k] for k in order])


SHARED = {
    "null descriptor": dict(m=None),
    "null cloud": dict(c=None),
    "negative S": dict(S=-1),
    "null ctrl": dict(ctrl=None),
    "null knots": dict(knots=None),
    "null valid": dict(valid=None),
    "degree 0": dict(degree=0),
    "degree 6": dict(degree=6, n_ctrl=8),
    "n_ctrl equal to the degree": dict(n_ctrl=3),
    "n_ctrl 65537": dict(n_ctrl=65537),
    "threshold NaN": dict(threshold=nan),
}
BAD_A = dict(SHARED, **{
    "null workspace": dict(workspace=None),
    "resolution 0": dict(resolution=0.0),
    "resolution negative": dict(resolution=-0.05),
    "resolution NaN": dict(resolution=nan),
    "resolution inf": dict(resolution=inf),
    "workspace one byte short": dict(workspace_bytes=None),
    "workspace of no bytes": dict(workspace_bytes=0),
    "workspace offset by 8 bytes": dict(workspace_offset=8, workspace_bytes=1 << 15),
})
BAD_B = dict(SHARED, **{
    "null t_free": dict(t_free=None),
    "null status": dict(status=None),
    "max_iter 0": dict(max_iter=0),
    "slack negative": dict(slack=-1.0),
    "slack NaN": dict(slack=nan),
    "look_ahead 0": dict(look_ahead=0.0),
    "look_ahead negative": dict(look_ahead=-0.05),
    "look_ahead NaN": dict(look_ahead=nan),
})


@pytest.mark.parametrize("case", sorted(BAD_A))
def test_sampled_entry_refuses_bad_arguments_before_any_device(case):
    from numbotics_amd import _lib
    lib = _lib.load()
    kw = dict(BAD_A[case])
    if case == "workspace one byte short":
        kw["workspace_bytes"] = lib.nbk_spline_cloud_workspace_bytes(4) - 1
    assert _call(lib, "a", **kw) == INVALID, case


@pytest.mark.parametrize("case", sorted(BAD_B))
def test_certified_entry_refuses_bad_arguments_before_any_device(case):
    from numbotics_amd import _lib
    assert _call(_lib.load(), "b", **BAD_B[case]) == INVALID, case


def test_no_trajectories_is_ok_at_once_and_the_rules_come_first():
    from numbotics_amd import _lib
    lib = _lib.load()
    assert _call(lib, "a", S=0, ctrl=None, knots=None, valid=None, workspace=None, workspace_bytes=0) == 0
    assert _call(lib, "a", S=0, resolution=0.0) == INVALID
    assert _call(lib, "a", S=0, degree=0) == INVALID
    assert _call(lib, "b", S=0, ctrl=None, knots=None, valid=None, t_free=None, status=None) == 0
    assert _call(lib, "b", S=0, look_ahead=inf) == 0
    assert _call(lib, "b", S=0, look_ahead=0.0) == INVALID
    assert _call(lib, "b", S=0, n_ctrl=3) == INVALID
    # too many trajectories: refused as unsupported, also without a device (the workspace is not even asked about)
    assert _call(lib, "a", S=2**26, workspace_bytes=0) == -4


# ---- the per-shape span bounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["c2", "tree"])
def test_shape_span_bounds(fresh_world, scene):
    from numbotics_amd.engine import spline_motion_bounds, spline_shape_motion_bounds, edge_shape_motion_bounds
    arm, chain, obs = tree_scene() if scene == "tree" else build_scene(scene)
    sm = arm.scene_model()
    one = cloud_model(sm, np.array([[0.3, 0.1, 0.2]]), 0.01)          # pair x = (robot shape x, the point)
    for k, n, knots in ((1, 2, None), (3, 6, None), (5, 9, None), (2, 6, np.array([0.0, 0.0, 0.0, 0.3, 0.3, 0.7, 1.0, 1.0, 1.0]))):
        knots = unit_knots(n, k) if knots is None else knots
        c = random_splines(chain, 5, n, 40 + k)
        mu = spline_shape_motion_bounds(sm, c, knots, k)
        assert mu.shape == (5, n - k, sm.n_rshapes) and mu.dtype == np.float64
        ref = spline_motion_bounds(one, c, knots, k)
        assert np.array_equal(mu.view(np.int64), ref.view(np.int64)), "shape bound and pair bound differ in their bits"
        empty = ~(knots[k:n] < knots[k + 1:n + 1])
        assert (mu[:, empty] == 0.0).all() and (mu[:, ~empty] > 0.0).any() and (mu >= 0.0).all()
        indep = motion_bounds_numpy(one, c, knots, k)
        np.testing.assert_allclose(mu, indep, rtol=1e-12, atol=0.0)
    # two control points, degree 1: the edge's bound, bit for bit
    s, g = random_edges(chain, 12, 5)
    mu = spline_shape_motion_bounds(sm, np.stack((s, g), axis=1), unit_knots(2, 1), 1)
    assert np.array_equal(mu[:, 0].view(np.int64), edge_shape_motion_bounds(sm, s, g).view(np.int64))


def test_shape_span_bounds_reject_bad_arguments(fresh_world):
    from numbotics_amd import _lib
    from numbotics_amd.engine import model_desc, spline_shape_motion_bounds
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    d, keep = model_desc(sm)
    fn = _lib.load().nbk_spline_shape_motion_bounds_host
    c = np.zeros((2, 6, sm.kin.n_q))
    kn = np.ascontiguousarray(unit_knots(6, 3), dtype=np.float64)
    mu = np.empty((2, 3, sm.n_rshapes))
    assert fn(C.byref(d), c.ctypes.data, 2, 6, 3, kn.ctypes.data, mu.ctypes.data) == 0 and (mu == 0.0).all()      # nothing moves
    assert fn(None, c.ctypes.data, 2, 6, 3, kn.ctypes.data, mu.ctypes.data) == INVALID
    assert fn(C.byref(d), c.ctypes.data, -1, 6, 3, kn.ctypes.data, mu.ctypes.data) == INVALID
    assert fn(C.byref(d), None, 2, 6, 3, kn.ctypes.data, mu.ctypes.data) == INVALID
    assert fn(C.byref(d), c.ctypes.data, 2, 6, 3, None, mu.ctypes.data) == INVALID
    assert fn(C.byref(d), c.ctypes.data, 2, 6, 3, kn.ctypes.data, None) == INVALID
    assert fn(C.byref(d), c.ctypes.data, 2, 6, 0, kn.ctypes.data, mu.ctypes.data) == INVALID
    assert fn(C.byref(d), c.ctypes.data, 2, 3, 3, kn.ctypes.data, mu.ctypes.data) == INVALID
    bad = np.ascontiguousarray(kn * 2.0)
    assert fn(C.byref(d), c.ctypes.data, 2, 6, 3, bad.ctypes.data, mu.ctypes.data) == INVALID
    assert fn(C.byref(d), None, 0, 6, 3, None, None) == 0
    with pytest.raises(ValueError):
        spline_shape_motion_bounds(sm, np.zeros((2, 6, sm.kin.n_q + 1)), kn, 3)
    with pytest.raises(ValueError):
        spline_shape_motion_bounds(sm, c, kn[:-1], 3)


# ---- the connectors' keyword, on a stub device ----------------------------------------------------------------------------------
class _Cloud:
    pass


class _Dev:
    """Records the calls; the scene's call returns three arrays, the cloud's call must get exactly those as ``out``."""

    def __init__(self):
        self.calls = []

    def _scene(self, name, ctrl, knots, degree, kw):
        S = ctrl.shape[0]
        out = tuple(np.zeros(S) + i for i in range(3))
        self.calls.append((name, ctrl, np.asarray(knots), degree, kw, out))
        return out

    def spline_validity(self, ctrl, knots, degree, resolution, **kw):
        return self._scene("spline_validity", ctrl, knots, degree, dict(kw, resolution=resolution))

    def spline_continuous(self, ctrl, knots, degree, **kw):
        return self._scene("spline_continuous", ctrl, knots, degree, kw)

    def _cloud(self, name, cloud, ctrl, knots, degree, kw):
        self.calls.append((name, cloud, ctrl, np.asarray(knots), degree, kw))
        for x in kw["out"]:
            x += 10.0                                    # "accumulates"
        return kw["out"]

    def cloud_spline_validity(self, cloud, ctrl, knots, degree, resolution, **kw):
        return self._cloud("cloud_spline_validity", cloud, ctrl, knots, degree, dict(kw, resolution=resolution))

    def cloud_spline_continuous(self, cloud, ctrl, knots, degree, **kw):
        return self._cloud("cloud_spline_continuous", cloud, ctrl, knots, degree, kw)


class _Arm:
    dof = 7

    def __init__(self):
        self.dev = _Dev()
        self.asked = []

    def _scene_device(self):
        return "sm", self.dev

    def _cloud_shapes(self, sm, links):
        assert sm == "sm"
        self.asked.append(links)
        return ["shapes without", links]


@pytest.mark.parametrize("kind", ["discrete", "continuous"])
def test_trajectory_methods_take_a_cloud_per_call(kind):
    import torch
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector, DiscreteConnector
    arm, scan = _Arm(), _Cloud()
    if kind == "discrete":
        conn = DiscreteConnector(ConnectorParams(arm=arm, resolution=0.02, collision_threshold=0.003, cloud_ignore_links=("base",)))
        scene_name, cloud_name = "spline_validity", "cloud_spline_validity"
    else:
        conn = ContinuousConnector(ConnectorParams(arm=arm, collision_threshold=0.003), max_iter=9, slack=1e-5,
                                   cloud_ignore_links=("base",), look_ahead=0.07)
        scene_name, cloud_name = "spline_continuous", "cloud_spline_continuous"
    ctrl = torch.zeros((3, 6, 7), dtype=torch.float64)               # a tensor stays where it is: nothing is staged by the connector
    # without a cloud: the scene's call alone, as before
    out = conn.validate_trajectories(ctrl, degree=3)
    assert [c[0] for c in arm.dev.calls] == [scene_name] and out is arm.dev.calls[0][-1]
    arm.dev.calls.clear()
    # with a cloud: the scene first, then the cloud into the same three arrays; the connector's own ignore list by default
    out = conn.validate_trajectories(ctrl, degree=3, cloud=scan)
    (n0, c0, k0, d0, kw0, out0), (n1, cl1, c1, k1, d1, kw1) = arm.dev.calls
    assert (n0, n1) == (scene_name, cloud_name) and cl1 is scan
    assert c0 is ctrl and c1 is ctrl and d0 == d1 == 3 and np.array_equal(k0, unit_knots(6, 3)) and np.array_equal(k1, k0)
    assert kw1["out"] is out0 and all(a is b for a, b in zip(out, out0))
    assert [float(x[0]) for x in out] == [10.0, 11.0, 12.0]
    assert arm.asked == [("base",)] and kw1["shapes"] == ["shapes without", ("base",)]
    assert kw1["threshold"] == kw0["threshold"] == 0.003
    if kind == "discrete":
        assert kw0["resolution"] == kw1["resolution"] == 0.02
    else:
        assert kw1["look_ahead"] == 0.07 and kw1["max_iter"] == kw0["max_iter"] == 9 and kw1["slack"] == kw0["slack"] == 1e-5
    # an ignore list given with the call wins, an empty one included
    arm.dev.calls.clear()
    conn.validate_trajectories(ctrl, degree=3, cloud=scan, cloud_ignore_links=())
    conn.validate_trajectories(ctrl, degree=3, cloud=scan, cloud_ignore_links=["wrist"])
    assert arm.asked[1:] == [(), ("wrist",)]


def test_calls_that_name_no_cloud_keep_their_refusals():
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector, DiscreteConnector
    arm, scan = _Arm(), _Cloud()
    dc = DiscreteConnector(ConnectorParams(arm=arm, cloud=scan))
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        dc.validate_trajectories(np.zeros((2, 4, 7)), degree=3)
    cc = ContinuousConnector(ConnectorParams(arm=arm), cloud=scan)
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        cc.validate_trajectory(unit_bspline(np.zeros((4, 7))))
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        ContinuousConnector(ConnectorParams(arm=arm, cloud=scan))
    assert arm.dev.calls == []
