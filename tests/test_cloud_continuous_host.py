"""Certified continuous edges against a point cloud, the part that needs no device: the per-shape motion bound
(nbk_edge_shape_motion_bounds_host) against the pair bound of the same shape with a world shape and against an independent NumPy
construction; the two entry points declared, bound and exported; the argument rules of nbk_edge_cloud_continuous_batch that are answered
before a device is looked for; the restatement's own soundness; and ContinuousConnector's constructor rules with a cloud."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from numbotics_amd.scenes import build_scene
from cloud_cases import cloud_model, scan
from continuous_ref import motion_bounds_numpy, random_edges, random_scene, tree_scene, FREE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
SCENES = ["c2", "tree", "rand3", "rand11", "rand29"]


def _scene(name, tmp_path):
    if name == "tree":
        return tree_scene()
    if name.startswith("rand"):
        built = random_scene(int(name[4:]), tmp_path)
        assert built is not None, f"random scene {name} has no joints or no pairs: pick another seed"
        return built
    return build_scene(name)


@pytest.mark.parametrize("scene", SCENES)
def test_shape_bound_is_the_pair_bound_against_a_world_shape(fresh_world, tmp_path, scene):
    from numbotics_amd.engine import edge_motion_bounds, edge_shape_motion_bounds
    arm, chain, obs = _scene(scene, tmp_path)
    sm = arm.scene_model()
    s, g = random_edges(chain, 12, 5)
    mu = edge_shape_motion_bounds(sm, s, g)
    assert mu.shape == (12, sm.n_rshapes) and mu.dtype == np.float64
    one = cloud_model(sm, np.array([[0.3, 0.1, 0.2]]), 0.01)          # pair x = (robot shape x, the point)
    assert one.n_pairs == sm.n_rshapes
    ref = edge_motion_bounds(one, s, g)
    assert np.array_equal(mu.view(np.int64), ref.view(np.int64)), "shape bound and pair bound differ in their bits"
    assert (mu >= 0.0).all() and (mu > 0.0).any()
    # a subset keeps its columns
    sub = cloud_model(sm, np.array([[0.3, 0.1, 0.2]]), 0.01, shapes=[sm.n_rshapes - 1, 0])
    assert np.array_equal(edge_motion_bounds(sub, s, g), mu[:, [0, sm.n_rshapes - 1]])
    # at most the independent construction's value, up to its own rounding
    indep = motion_bounds_numpy(one, s, g)
    assert (mu <= indep * (1.0 + 1e-12)).all()
    np.testing.assert_allclose(mu, indep, rtol=1e-12, atol=0.0)


def test_symbols_are_declared_bound_and_exported():
    from numbotics_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "nbk.h")).read()
    declared = set(re.findall(r"\b(nbk_[a-z_]+)\s*\(", header))
    for s in ("nbk_edge_cloud_continuous_batch", "nbk_edge_shape_motion_bounds_host"):
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    assert len(lib.nbk_edge_cloud_continuous_batch.argtypes) == 19
    assert len(lib.nbk_edge_shape_motion_bounds_host.argtypes) == 5


ORDER = ("m", "c", "starts", "goals", "dist", "E", "max_distance", "mode", "threshold", "max_iter", "slack", "look_ahead", "shape_bits",
         "accumulate", "valid", "end", "t_free", "status", "stream")


def _call(lib, **kw):
    """nbk_edge_cloud_continuous_batch with arguments that pass every rule, except those given.  The descriptor and the cloud are
    stand-ins (zeroed memory, never dereferenced before the rules are through), the arrays are host memory never touched."""
    fake = (C.c_char * 4096)()
    mem = np.zeros((1 << 12,), dtype=np.uint8)
    base = mem.ctypes.data
    a = dict(m=C.addressof(fake), c=C.addressof(fake), starts=base, goals=base, dist=None, E=4, max_distance=0.25, mode=0, threshold=0.0,
             max_iter=64, slack=1e-6, look_ahead=0.05, shape_bits=None, accumulate=0, valid=base, end=None, t_free=base, status=base,
             stream=None)
    a.update(kw)
    keep = (fake, mem)                                                                        # noqa: F841
    return lib.nbk_edge_cloud_continuous_batch(*[a[k] for k in ORDER])


nan = float("nan")
BAD = {
    "null descriptor": dict(m=None),
    "null cloud": dict(c=None),
    "negative E": dict(E=-1),
    "null starts": dict(starts=None),
    "null goals": dict(goals=None),
    "null valid": dict(valid=None),
    "null t_free": dict(t_free=None),
    "null status": dict(status=None),
    "max_iter 0": dict(max_iter=0),
    "slack negative": dict(slack=-1.0),
    "slack NaN": dict(slack=nan),
    "threshold NaN": dict(threshold=nan),
    "max_distance 0": dict(max_distance=0.0),
    "max_distance NaN": dict(max_distance=nan),
    "mode 2": dict(mode=2),
    "mode -1": dict(mode=-1),
    "look_ahead 0": dict(look_ahead=0.0),
    "look_ahead negative": dict(look_ahead=-0.05),
    "look_ahead NaN": dict(look_ahead=nan),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_refuses_bad_arguments_before_any_device(case):
    from numbotics_amd import _lib
    assert _call(_lib.load(), **BAD[case]) == INVALID, case


def test_no_edges_is_ok_at_once_and_the_rules_come_first():
    from numbotics_amd import _lib
    lib = _lib.load()
    assert _call(lib, E=0, starts=None, goals=None, valid=None, t_free=None, status=None) == 0
    assert _call(lib, E=0, look_ahead=float("inf")) == 0
    assert _call(lib, E=0, look_ahead=0.0) == INVALID
    assert _call(lib, E=0, max_iter=0) == INVALID


def test_shape_motion_bounds_host_rejects_bad_arguments(fresh_world):
    from numbotics_amd import _lib
    from numbotics_amd.engine import model_desc, edge_shape_motion_bounds
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    d, keep = model_desc(sm)
    lib = _lib.load()
    s = np.zeros((2, sm.kin.n_q))
    mu = np.empty((2, sm.n_rshapes))
    fn = lib.nbk_edge_shape_motion_bounds_host
    assert fn(C.byref(d), s.ctypes.data, s.ctypes.data, 2, mu.ctypes.data) == 0 and (mu == 0.0).all()      # start == goal: nothing moves
    assert fn(None, s.ctypes.data, s.ctypes.data, 2, mu.ctypes.data) == INVALID
    assert fn(C.byref(d), s.ctypes.data, s.ctypes.data, -1, mu.ctypes.data) == INVALID
    assert fn(C.byref(d), None, s.ctypes.data, 2, mu.ctypes.data) == INVALID
    assert fn(C.byref(d), s.ctypes.data, s.ctypes.data, 2, None) == INVALID
    assert fn(C.byref(d), None, None, 0, None) == 0
    fr = np.array(sm.rshape_frame, dtype=np.int32)
    fr[0] = sm.kin.n_joints                                # out of range
    d.rshape_frame = fr.ctypes.data
    assert fn(C.byref(d), s.ctypes.data, s.ctypes.data, 2, mu.ctypes.data) == INVALID
    with pytest.raises(ValueError):
        edge_shape_motion_bounds(sm, np.zeros((2, sm.kin.n_q)), np.zeros((3, sm.kin.n_q)))


def test_restatement_is_sound_and_takes_every_exit(fresh_world):
    """The restatement alone, on the CPU: FREE edges are free in a dense sampling, the cut never changes a sound verdict into an
    unsound one, and look_ahead = inf differs from 0.03 only in the steps it takes."""
    from cloud_continuous_ref import reference_cloud_continuous, dense_cloud_min_distance, EXIT_INF, EXIT_CAP
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    pts, r = scan(200, seed=200), 0.01
    shapes = list(range(1, sm.n_rshapes))
    s, g = random_edges(chain, 24, 23, scale=0.3)
    out = {}
    for la in (0.03, np.inf):
        valid, end, t_free, status, stop, st, exits = reference_cloud_continuous(sm, pts, r, s, g, 1.0, look_ahead=la, shapes=shapes)
        assert valid.any() and (~valid).any()
        assert np.array_equal(valid, status == FREE)
        assert exits[EXIT_INF] > 0
        assert (exits[EXIT_CAP] > 0) == (la == 0.03)
        for e in np.nonzero(valid)[0][:6]:
            assert dense_cloud_min_distance(sm, pts, r, shapes, s[e], g[e], n=400) > 0.0
        out[la] = status
    assert not ((out[0.03] == FREE) & (out[np.inf] != FREE) & (out[np.inf] != 2)).any(), "FREE under the cut, COLLISION without it"


class _Stub:
    """Stands in for an arm and for a cloud: any use of it is an error."""
    dof = 7

    def __getattr__(self, name):
        raise AssertionError(f"touched {name} before the refusal")


def test_continuous_connector_constructor_rules_with_a_cloud():
    from numbotics_amd.planning import unit_bspline
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector
    from numbotics_amd import engine
    p = ConnectorParams(arm=_Stub())
    cc = ContinuousConnector(p, cloud=_Stub(), cloud_ignore_links=("base",))
    assert cc.cloud is not None and cc.cloud_ignore_links == ("base",) and cc.look_ahead == engine.CLOUD_LOOK_AHEAD
    assert ContinuousConnector(p, cloud=_Stub(), look_ahead=float("inf")).look_ahead == float("inf")
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        cc.validate_trajectories(np.zeros((2, 4, 7)), degree=3)
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        cc.validate_trajectory(unit_bspline(np.zeros((4, 7))))
    with pytest.raises(ValueError, match="validity_checker"):
        ContinuousConnector(ConnectorParams(arm=_Stub(), validity_checker=lambda q: 1.0), cloud=_Stub())
    with pytest.raises(ValueError, match="arm"):
        ContinuousConnector(ConnectorParams(validity_checker=lambda q: 1.0), cloud=_Stub())
    with pytest.raises(ValueError, match="trajectory"):
        ContinuousConnector(ConnectorParams(arm=_Stub(), trajectory_func=lambda x, y: None), cloud=_Stub())
    for la in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="look_ahead"):
            ContinuousConnector(p, cloud=_Stub(), look_ahead=la)
    with pytest.raises(ValueError, match="do not see point clouds yet"):            # the params' own cloud keeps being refused
        ContinuousConnector(ConnectorParams(arm=_Stub(), cloud=_Stub()), cloud=_Stub())
    plain = ContinuousConnector(p)                              # without a cloud: as before
    assert plain.cloud is None
