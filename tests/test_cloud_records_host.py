"""Proximity records against a point cloud, the part that needs no device: the header / binding agreement of nbk_records_cloud_batch,
its argument rules (answered before any device is looked for), the Python wrappers' argument errors, and a sanity check of the
reference the GPU tests compare with (tests/cloud_records_cases.py): the winner's row is the gradient of the per-shape clearance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cloud_cases import scan
from cloud_records_cases import Raw, cut, second_gap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
SYMBOL = "nbk_records_cloud_batch"


def test_records_symbol_is_declared_bound_and_exported():
    from numbotics_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "nbk.h")).read()
    declared = set(re.findall(r"\b(nbk_[a-z_]+)\s*\(", header))
    assert SYMBOL in declared
    assert SYMBOL in _lib.SYMBOLS
    assert hasattr(lib, SYMBOL)
    assert len(getattr(lib, SYMBOL).argtypes) == 13


def _call(lib, m=1, c=1, q=1, B=64, d_max=0.05, dist=1, per_shape=0):
    """The entry with stand-in handles: a rule that refuses the call reads none of them (there is no device to make real ones)."""
    buf = np.zeros(64 * 16)
    h = lambda on: buf.ctypes.data if on else None
    return lib.nbk_records_cloud_batch(h(m), h(c), h(q), B, d_max, None, per_shape, h(dist), None, None, None, None, None)


@pytest.mark.parametrize("per_shape", [0, 1])
def test_records_argument_rules_are_answered_before_any_device(per_shape):
    from numbotics_amd import _lib
    lib = _lib.load()
    assert _call(lib, m=0, per_shape=per_shape) == INVALID
    assert _call(lib, c=0, per_shape=per_shape) == INVALID
    assert _call(lib, q=0, per_shape=per_shape) == INVALID
    assert _call(lib, dist=0, per_shape=per_shape) == INVALID
    assert _call(lib, B=-1, per_shape=per_shape) == INVALID
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert _call(lib, d_max=bad, per_shape=per_shape) == INVALID
        assert _call(lib, d_max=bad, B=0, per_shape=per_shape) == INVALID
    assert _call(lib, m=0, B=0, per_shape=per_shape) == INVALID
    assert _call(lib, c=0, B=0, per_shape=per_shape) == INVALID
    # B = 0: nothing to do, whatever the other pointers are
    assert _call(lib, B=0, per_shape=per_shape) == OK
    assert _call(lib, B=0, q=0, dist=0, per_shape=per_shape) == OK


def test_python_wrappers_refuse_bad_arguments_before_the_device(fresh_world):
    from numbotics_amd.scenes import build_scene
    from numbotics_amd.engine import DeviceModel
    from numbotics_amd.planning import safe_sets
    arm, chain, keep = build_scene("c1")
    sm = arm.scene_model()
    cloud = object()                                          # never looked at: every call below fails on its arguments
    q = np.zeros((5, arm.dof))
    with pytest.raises(ValueError):
        arm.cloud_proximity_jacobians(np.zeros((5, arm.dof + 1)), cloud, 0.05)
    with pytest.raises(ValueError):
        arm.cloud_proximity_jacobians(q, cloud, 0.05, ignore_links=["no_such_link"])
    with pytest.raises(ValueError):
        arm.cloud_proximity_jacobians(q, cloud, 0.05, ignore_links=["no_such_link"], per_shape=True)
    with pytest.raises(ValueError):
        arm.cloud_closest_to(q, cloud, 0.05)                  # one (dof,) configuration only
    with pytest.raises(ValueError):
        arm.cloud_closest_to(np.zeros(arm.dof + 1), cloud, 0.05)
    with pytest.raises(ValueError):
        arm.cloud_closest_to(q[0], cloud, 0.05, ignore_links=["no_such_link"])
    with pytest.raises(ValueError):
        safe_sets.cloud_distance_and_gradient(arm, q, cloud, 0.05, link="no_such_link")
    with pytest.raises(ValueError):
        safe_sets.cloud_distance_and_gradient(arm, q, cloud, 0.05, ignore_links=["no_such_link"])
    # a shape out of range: DeviceModel.cloud_records checks its selection first (an object without a handle: no device was asked)
    dev = DeviceModel.__new__(DeviceModel)
    dev.scene, dev.n_q = sm, arm.dof
    for shapes in ([sm.n_rshapes], [-1], [0, 1, 10 ** 6]):
        with pytest.raises(ValueError, match="out of range"):
            dev.cloud_records(cloud, q, 0.05, shapes=shapes)


@pytest.mark.parametrize("name", ["c1", "c2m"])
def test_reference_row_is_the_gradient_of_the_per_shape_clearance(fresh_world, name):
    """Central differences (h = 1e-4) of the oracle's per-shape clearance min_i d(s, i) against the winner's row, on the records
    where the clearance is smooth: distance > 5e-3 (no contact), below d_max = 0.1, and the second-nearest point at least 5e-3
    farther (the argmin does not switch within h).  Bound 2e-5, the figure of tests/test_oracle_proximity.py; measured: 8.6e-7."""
    from oracle.cpu_oracle import Oracle
    from cloud_cases import cloud_model
    from numbotics_amd.scenes import build_scene, sample_q
    arm, chain, keep = build_scene(name)
    sm = arm.scene_model()
    q = sample_q(chain, 64, seed=3)
    pts = scan(300, seed=300)
    r, d_max, h = 0.01, 0.1, 1e-4
    shapes = list(range(1, sm.n_rshapes))
    raw = Raw(sm, pts, r, q, shapes)
    dist, shape, point, wit, rows = cut(raw, d_max, per_shape=True)
    assert not np.isnan(wit[np.isfinite(dist)]).any() and not np.isnan(rows).any()
    near = np.isfinite(dist)
    keep_ = near & (dist > 5e-3) & (second_gap(raw) > 5e-3)
    share = keep_.sum() / near.sum()
    print(f"{name}: {near.sum()} near records, {share:.2f} of them kept")
    assert share >= 0.20, share
    B, S, nq = raw.B, raw.S, raw.n_q
    orc = Oracle(cloud_model(sm, pts, r, shapes))
    step = h * np.eye(nq)
    qq = np.concatenate([q[:, None, :] + step[None], q[:, None, :] - step[None]], axis=1).reshape(B * 2 * nq, nq)
    f = orc.pair_distances(qq).reshape(B, 2, nq, S, raw.N).min(axis=4)              # per-shape clearance at q +- h e_j
    grad = np.transpose((f[:, 0] - f[:, 1]) / (2.0 * h), (0, 2, 1))                # (B, S, nq)
    err = np.abs(grad - rows)[keep_]
    print(f"{name}: worst error {err.max():.3g}")
    assert err.max() <= 2e-5, err.max()
