"""Sampled edges against a point cloud, the part that needs no device: the two entry points are declared, bound and exported; the
workspace size; every argument rule of nbk_edge_cloud_validity_batch that is answered before a device is looked for; and the
connectors' refusals (a cloud without an arm; trajectories and certified checks with a cloud)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
SYMBOLS = ("nbk_edge_cloud_workspace_bytes", "nbk_edge_cloud_validity_batch")


def test_edge_cloud_symbols_are_declared_bound_and_exported():
    from numbotics_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "nbk.h")).read()
    declared = set(re.findall(r"\b(nbk_[a-z_]+)\s*\(", header))
    for s in SYMBOLS:
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    assert len(lib.nbk_edge_cloud_validity_batch.argtypes) == 18
    assert "#define NBK_ABI_VERSION 2" in header


def test_edge_cloud_workspace_bytes():
    from numbotics_amd import _lib
    from numbotics_amd.engine import DeviceModel
    size = _lib.load().nbk_edge_cloud_workspace_bytes
    assert size(0) >= 0
    sizes = [size(E) for E in (0, 1, 2, 7, 8, 9, 63, 64, 65, 1000, 10**6, 2**31 - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert size(10**6) <= 64 * 10**6, "a few tens of bytes per edge"
    assert size(10**6) >= 40 * 10**6, "plan (3 doubles), count and offset of every edge"
    for E in (-1, -2**31, -2**62):
        assert size(E) < 0
    assert DeviceModel.cloud_edge_workspace_bytes(1000) == size(1000)


def _call(lib, **kw):
    """nbk_edge_cloud_validity_batch with arguments that pass every rule, except those given.  The descriptor and the cloud are
    stand-ins (zeroed memory, never dereferenced before the rules are through), the arrays are host memory never touched."""
    E = kw.get("E", 4)
    fake = (C.c_char * 4096)()
    mem = np.zeros((1 << 16,), dtype=np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 64
    a = dict(m=C.addressof(fake), c=C.addressof(fake), starts=base, goals=base, dist=None, E=E, resolution=0.05, max_distance=0.25, mode=0,
             threshold=0.0, shape_bits=None, accumulate=0, valid=base, end=None, n_samples=None, workspace=base,
             workspace_bytes=lib.nbk_edge_cloud_workspace_bytes(max(E, 0)), stream=None)
    if "workspace_offset" in kw:
        a["workspace"] = base + kw.pop("workspace_offset")
    a.update(kw)
    keep = (fake, mem)                                                                        # noqa: F841
    return lib.nbk_edge_cloud_validity_batch(*[a[k] for k in ("m", "c", "starts", "goals", "dist", "E", "resolution", "max_distance", "mode",
                                                               "threshold", "shape_bits", "accumulate", "valid", "end", "n_samples",
                                                               "workspace", "workspace_bytes", "stream")])


BAD = {
    "null descriptor": dict(m=None),
    "null cloud": dict(c=None),
    "negative E": dict(E=-1),
    "null starts": dict(starts=None),
    "null goals": dict(goals=None),
    "null valid": dict(valid=None),
    "null workspace": dict(workspace=None),
    "resolution 0": dict(resolution=0.0),
    "resolution negative": dict(resolution=-0.05),
    "resolution NaN": dict(resolution=float("nan")),
    "max_distance 0": dict(max_distance=0.0),
    "max_distance NaN": dict(max_distance=float("nan")),
    "mode 2": dict(mode=2),
    "mode -1": dict(mode=-1),
    "threshold NaN": dict(threshold=float("nan")),
    "workspace one byte short": dict(workspace_bytes=None),
    "workspace of no bytes": dict(workspace_bytes=0),
    "workspace offset by 8 bytes": dict(workspace_offset=8, workspace_bytes=1 << 15),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_edge_cloud_refuses_bad_arguments_before_any_device(case):
    from numbotics_amd import _lib
    lib = _lib.load()
    kw = dict(BAD[case])
    if case == "workspace one byte short":
        kw["workspace_bytes"] = lib.nbk_edge_cloud_workspace_bytes(4) - 1
    assert _call(lib, **kw) == INVALID, case


def test_edge_cloud_no_edges_is_ok_at_once():
    from numbotics_amd import _lib
    lib = _lib.load()
    assert _call(lib, E=0, starts=None, goals=None, valid=None, workspace=None, workspace_bytes=0) == 0
    assert _call(lib, E=0, resolution=0.0) == INVALID, "the rules come first"


class _Stub:
    """Stands in for an arm and for a cloud: any use of it is an error."""
    dof = 7

    def __getattr__(self, name):
        raise AssertionError(f"touched {name} before the refusal")


def test_connector_params_with_a_cloud_need_an_arm():
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams
    with pytest.raises(ValueError, match="arm"):
        ConnectorParams(validity_checker=lambda q: True, cloud=_Stub())
    p = ConnectorParams(arm=_Stub(), cloud=_Stub(), cloud_ignore_links=("base",))
    assert p.cloud_ignore_links == ("base",)
    assert ConnectorParams(arm=_Stub()).cloud is None and ConnectorParams(arm=_Stub()).cloud_ignore_links == ()


def test_trajectories_and_certified_checks_refuse_a_cloud():
    from numbotics_amd.planning import unit_bspline
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, DiscreteConnector, ContinuousConnector
    p = ConnectorParams(arm=_Stub(), cloud=_Stub())
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        ContinuousConnector(p)
    dc = DiscreteConnector(p)
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        dc.validate_trajectories(np.zeros((2, 4, 7)), degree=3)
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        dc.validate_trajectory(unit_bspline(np.zeros((4, 7))))
    ContinuousConnector(ConnectorParams(arm=_Stub()))           # without a cloud: as before
