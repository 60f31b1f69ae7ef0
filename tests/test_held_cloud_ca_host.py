"""Certified checks of the held object against point clouds, the part that needs no device: the host twins of the per-shape motion
bound against the scene's own routine on ``held_robot_model``, the argument rules the two device entries answer before any device is
touched, the connector's rules, and -- by the reference alone -- the conditions the GPU tests (tests/test_gpu_held_cloud_ca.py) rely
on: at least 10 % FREE, at least 10 % COLLISION and at most 5 % UNDECIDED in every set of 100 or more trajectories."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from numbotics_amd import _lib
from numbotics_amd.engine import edge_shape_motion_bounds, spline_shape_motion_bounds
import held_cases as hc
import held_cloud_cases as hcc
import held_cloud_ca_cases as hca
import held_traj_cases as ht

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nbk_edge_held_cloud_continuous_batch", "nbk_spline_held_cloud_continuous_batch", "nbk_edge_held_shape_motion_bounds_host",
           "nbk_spline_held_shape_motion_bounds_host")
nan, inf = float("nan"), float("inf")


def test_symbols_declared_and_bound():
    with open(os.path.join(ROOT, "include", "nbk.h")) as f:
        text = f.read()
    declared = set(re.findall(r"\b(nbk_\w+)\s*\(", text))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/nbk.h"
        assert s in _lib.SYMBOLS, f"{s} is not listed in _lib.SYMBOLS"
        assert hasattr(lib, s), f"libnbk.so lacks {s}"
        assert getattr(lib, s).argtypes is not None, f"{s} has no argtypes"
    assert re.search(r"#define\s+NBK_ABI_VERSION\s+2\b", text), "additions only: the ABI version stays 2"


# ---- the motion bound ----------------------------------------------------------------------------------------------------------------
def _fixture(name):
    """-> (the scene's namespace, (starts, goals) of 40 edges): the Kinova arm with the gripper box (H = 1) or the eight parts (H = 8),
    or the prismatic-below-revolute tree of tests/test_held_traj_host.py (H = 1)."""
    if name == "tree":
        x = ht.scene("tree")
        kin = x.sm.kin
        path, f = [], x.spec.frame
        while f >= 0:
            path.append(int(f))
            f = int(kin.joint_parent[f])
        types_ = [int(kin.joint_type[j]) for j in path[::-1]]
        assert 1 in types_[1:] and 0 in types_[:types_.index(1, 1)], f"a prismatic joint below a revolute one on the holding path: {types_}"
        return x, ht.edges(x, 40)
    x = hca.scene("c2", att=hca.eight_att if name == "eight" else None)
    return x, hca.edges(x, 40)


@pytest.mark.parametrize("name", ("box", "eight", "tree"))
def test_shape_motion_bounds_equal_the_scene_routine(fresh_world, name):
    """The host twins give, held shape by held shape, the bits ``edge_shape_motion_bounds`` / ``spline_shape_motion_bounds`` give for
    robot shapes S .. S+H-1 of ``held_robot_model``, with the stored grasp and with another."""
    from numbotics_amd.engine import held_edge_shape_motion_bounds, held_spline_shape_motion_bounds
    x, (s, g) = _fixture(name)
    S, H = x.sm.n_rshapes, int(len(x.spec.shape_type))
    assert H == (8 if name == "eight" else 1)
    rng = np.random.default_rng(11)
    for G in (None, x.spec.G @ hc.rot_pose(rng, 0.4, 0.03)):
        hm, shapes = hcc.held_robot_model(x.sm, x.spec, G)
        assert shapes == list(range(S, S + H))
        ref = edge_shape_motion_bounds(hm, s, g)[:, S:S + H]
        got = held_edge_shape_motion_bounds(x.sm, x.spec, s, g, G=G)
        assert got.shape == (40, H) and (ref > 0.0).all()
        ht.assert_bits(got, ref, f"{name} edge mu")
        if H == 8:
            assert len({ref[0, h] for h in range(8)}) >= 2, "the held shapes' bounds differ"
        for degree in (1, 3, 5):
            ctrl, knots = ht.splines(x, degree, S=12, n=8)
            knots = knots.copy()
            knots[degree + 2] = knots[degree + 1]           # a repeated interior knot: an empty span, whose entries are 0
            assert (np.diff(knots[degree:8 + 1]) == 0.0).sum() == 1
            ref = spline_shape_motion_bounds(hm, ctrl, knots, degree)[..., S:S + H]
            got = held_spline_shape_motion_bounds(x.sm, x.spec, ctrl, knots, degree, G=G)
            assert got.shape == (12, 8 - degree, H)
            ht.assert_bits(got, ref, f"{name} spline mu, degree {degree}")
            empty = np.flatnonzero(np.diff(knots[degree:8 + 1]) == 0.0)
            assert (got[:, empty, :] == 0.0).all() and (np.delete(got, empty, axis=1) > 0.0).all()


def test_host_twin_argument_rules(fresh_world):
    """The held arguments are nbk_held_create's: a bad frame, a non-finite grasp and a hull are answered as there."""
    from numbotics_amd.engine import held_edge_shape_motion_bounds, model_desc
    x = hca.scene("c2")
    s, g = hca.edges(x, 4)
    with pytest.raises(_lib.NbkError):
        held_edge_shape_motion_bounds(x.sm, x.spec, s, g, G=np.full((4, 4), np.nan))
    d, keep = model_desc(x.sm)
    a = np.eye(4)[:3].reshape(12).copy()
    one = np.array([0.05, 0.0, 0.0, 0.0])
    mu = np.zeros(64)
    lib = _lib.load()
    call = lambda frame, typ, E=4: lib.nbk_edge_held_shape_motion_bounds_host(       # noqa: E731
        C.byref(d), frame, a.ctypes.data, a.ctypes.data, 1, np.array([typ], dtype=np.int32).ctypes.data, a.ctypes.data, one.ctypes.data,
        s.ctypes.data, g.ctypes.data, E, mu.ctypes.data)
    assert call(0, 0) == 0 and (mu[:4] > 0.0).all()
    assert call(0, 0, E=0) == 0
    assert call(0, 0, E=-1) == -1
    assert call(x.sm.kin.n_joints, 0) == -1
    assert call(0, 5) == -4, "a held hull is unsupported"
    assert call(0, 4) == -1, "a held plane is no shape"
    assert lib.nbk_edge_held_shape_motion_bounds_host(None, 0, a.ctypes.data, a.ctypes.data, 1, a.ctypes.data, a.ctypes.data,
                                                      a.ctypes.data, None, None, 0, None) == -1
    assert lib.nbk_spline_held_shape_motion_bounds_host(None, 0, a.ctypes.data, a.ctypes.data, 1, a.ctypes.data, a.ctypes.data,
                                                        a.ctypes.data, None, 0, 6, 3, None, None) == -1
    knots = np.array([0, 0, 0, 0, 0.5, 0.5, 1, 1, 1, 1], dtype=np.float64)
    ctrl = np.zeros((1, 6, x.sm.kin.n_q))
    spl = lambda n, k, kn=knots: lib.nbk_spline_held_shape_motion_bounds_host(       # noqa: E731
        C.byref(d), 0, a.ctypes.data, a.ctypes.data, 1, np.array([0], dtype=np.int32).ctypes.data, a.ctypes.data, one.ctypes.data,
        ctrl.ctypes.data, 1, n, k, kn.ctypes.data, mu.ctypes.data)
    assert spl(6, 3) == 0
    assert spl(6, 0) == -1 and spl(6, 6) == -1 and spl(3, 3) == -1
    assert spl(6, 3, knots[::-1].copy()) == -1, "knots that decrease"
    del keep


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
EDGE_ORDER = ("m", "held", "c", "starts", "goals", "dist", "E", "max_distance", "mode", "threshold", "max_iter", "slack", "look_ahead",
              "grasp", "accumulate", "valid", "end", "t_free", "status", "stream")
SPLINE_ORDER = ("m", "held", "c", "ctrl", "S", "n_ctrl", "degree", "knots", "threshold", "max_iter", "slack", "look_ahead", "grasp",
                "accumulate", "valid", "t_free", "status", "stream")


def _buffers():
    """Non-null stand-ins (tests/test_held_cloud_host.py): ``fake`` (zeroed) for the three handles -- a held object whose descriptor
    field reads null is "made against another descriptor" --, ``base`` an aligned address for every array."""
    fake = (C.c_char * 4096)()
    other = (C.c_char * 4096)()
    mem = np.zeros((1 << 16,), dtype=np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 64
    return C.addressof(fake), C.addressof(other), base, (fake, other, mem)


def _traj(lib, which, n=4, **kw):
    f, o, base, keep = _buffers()
    a = dict(m=f, held=o, c=f, threshold=0.0, max_iter=64, slack=1e-6, look_ahead=inf, grasp=None, accumulate=0, valid=base,
             t_free=base, status=base, stream=None)
    if which == "edges":
        a.update(starts=base, goals=base, dist=None, E=n, max_distance=0.25, mode=0, end=None)
    else:
        a.update(ctrl=base, S=n, n_ctrl=6, degree=3, knots=base)
    a.update(kw)
    fn, order = ((lib.nbk_edge_held_cloud_continuous_batch, EDGE_ORDER) if which == "edges" else
                 (lib.nbk_spline_held_cloud_continuous_batch, SPLINE_ORDER))
    return fn(*[a[k] for k in order])


def test_device_entries_argument_rules_need_no_device():
    lib = _lib.load()
    shared = {"null descriptor": dict(m=None), "null held object": dict(held=None), "null cloud": dict(c=None), "null valid": dict(valid=None),
              "null t_free": dict(t_free=None), "null status": dict(status=None), "NaN threshold": dict(threshold=nan),
              "max_iter 0": dict(max_iter=0), "negative slack": dict(slack=-1e-9), "NaN slack": dict(slack=nan),
              "look_ahead 0": dict(look_ahead=0.0), "look_ahead NaN": dict(look_ahead=nan), "negative look_ahead": dict(look_ahead=-0.05),
              "look_ahead -inf": dict(look_ahead=-inf)}
    edges = dict(shared, **{"negative E": dict(E=-1), "null starts": dict(starts=None), "null goals": dict(goals=None), "mode 2": dict(mode=2),
                            "mode -1": dict(mode=-1), "max_distance 0": dict(max_distance=0.0), "max_distance NaN": dict(max_distance=nan)})
    splines = dict(shared, **{"negative S": dict(S=-1), "null ctrl": dict(ctrl=None), "null knots": dict(knots=None), "degree 0": dict(degree=0),
                              "degree 6": dict(degree=6, n_ctrl=8), "n_ctrl equal to the degree": dict(n_ctrl=3)})
    for which, cases in (("edges", edges), ("splines", splines)):
        for what, kw in cases.items():
            assert _traj(lib, which, **kw) == -1, f"{which}: {what}"
        assert _traj(lib, which, n=0) == 0, f"{which}: nothing to do is answered before the handles are looked at"
        assert _traj(lib, which, n=0, valid=None, t_free=None, status=None) == 0
        assert _traj(lib, which, n=2**31) == -4, f"{which}: 2^31 trajectories are unsupported, without a device"
        # past its own rules the call asks whose the held object is, before any device: the stand-in belongs to no descriptor
        for kw in (dict(), dict(look_ahead=0.05), dict(n=2**31 - 1), dict(accumulate=1)):
            assert _traj(lib, which, **kw) == -1 and "another descriptor" in lib.nbk_last_error().decode(), (which, kw)
    base = _buffers()[2]
    assert _traj(lib, "edges", grasp=base) == -1 and "another descriptor" in lib.nbk_last_error().decode()


# ---- the connector -------------------------------------------------------------------------------------------------------------------
def test_connector_rules(fresh_world):
    import inspect
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector
    x = hca.scene("c2")
    cloud = object()                                             # (no rule below looks into it)
    p = ConnectorParams(arm=x.arm)
    assert inspect.signature(ContinuousConnector.__init__).parameters["attached_sees_cloud"].default is False
    assert ContinuousConnector(p).attached_sees_cloud is False
    assert ContinuousConnector(p, cloud=cloud, attached=x.att).attached_sees_cloud is False, "the default stays False"
    for kw in (dict(), dict(cloud=cloud), dict(attached=x.att)):
        with pytest.raises(ValueError, match=r"attached_sees_cloud needs ContinuousConnector\(cloud=\.\.\., attached=\.\.\.\)"):
            ContinuousConnector(p, attached_sees_cloud=True, **kw)
    con = ContinuousConnector(p, cloud=cloud, attached=x.att, attached_sees_cloud=True)
    assert con.attached_sees_cloud is True and con.cloud is cloud and con.attached is x.att
    # the params' flag stays refused here, with its message
    q = ConnectorParams(arm=x.arm, cloud=cloud, attached=x.att, attached_sees_cloud=True)
    with pytest.raises(ValueError, match="certified held-object checks do not see point clouds yet"):
        ContinuousConnector(q)
    with pytest.raises(ValueError, match="certified held-object checks do not see point clouds yet"):
        ContinuousConnector(q, cloud=cloud, attached=x.att, attached_sees_cloud=True)
    # a trajectory call that names no cloud still raises
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        con.validate_trajectories(x.q[None, :4], degree=1)
    # the flag needs what a cloud and a held object need
    with pytest.raises(ValueError):
        ContinuousConnector(ConnectorParams(validity_checker=lambda q: 1.0), cloud=cloud, attached=x.att, attached_sees_cloud=True)


# ---- the conditions of the GPU tests' inputs, by the reference alone ----------------------------------------------------------------------
@pytest.mark.parametrize("scan", ("dense", "sparse"))
def test_fixture_conditions_edges(fresh_world, scan):
    """Reference, 200 edges, (FREE, COLLISION, UNDECIDED): every set has at least 20 / 20 / at most 10; look_ahead = 0.05 takes the
    cap exit, look_ahead = inf the +inf exit."""
    from cloud_continuous_ref import EXIT_CAP, EXIT_INF
    from numbotics_amd.engine import held_edge_shape_motion_bounds
    x = hca.scene("c2")
    # the bounds the references advance with are the held routine's, on these very edges
    hm, shapes = hcc.held_robot_model(x.sm, x.spec)
    ht.assert_bits(held_edge_shape_motion_bounds(x.sm, x.spec, *hca.edges(x)), edge_shape_motion_bounds(hm, *hca.edges(x))[:, shapes],
                   "the fixture's edge mu")
    for mode in ("connect", "steer"):
        for thr in hca.THRESHOLDS:
            for la in hca.LOOK_AHEADS:
                ref = hca.edge_ref(x, "c2", scan, mode, thr, la)
                print(f"{scan} {mode} thr={thr} look_ahead={la}: {hca.shares(ref[3])}, exits {ref[6].tolist()}")
                hca.assert_shares(ref[3], f"{scan} {mode} thr={thr} look_ahead={la}")
                assert ref[6][EXIT_INF] > 0
                assert (ref[6][EXIT_CAP] > 0) == (la == 0.05)
    s, g = hca.edges(x)
    import continuous_ref
    Tf = np.array([continuous_ref.edge_span(s[e], g[e], None, hca.MAXD_STEER, "steer")[1] for e in range(s.shape[0])])
    assert (Tf < 1.0).sum() >= 20 and (Tf == 1.0).sum() >= 20, "steer cuts some edges and leaves others whole"


@pytest.mark.parametrize("degree", (1, 2, 3, 4, 5))
def test_fixture_conditions_splines(fresh_world, degree):
    from numbotics_amd.engine import held_spline_shape_motion_bounds
    x = hca.scene("c2")
    hm, shapes = hcc.held_robot_model(x.sm, x.spec)
    ctrl, knots = hca.splines(x, degree)
    ht.assert_bits(held_spline_shape_motion_bounds(x.sm, x.spec, ctrl, knots, degree),
                   spline_shape_motion_bounds(hm, ctrl, knots, degree)[..., shapes], "the fixture's spline mu")
    for scan in ("dense", "sparse"):
        for thr in hca.THRESHOLDS:
            ref = hca.spline_ref(x, "c2", scan, degree, thr)
            print(f"degree {degree} {scan} thr={thr}: {hca.shares(ref[2])}, exits {ref[5].tolist()}")
            hca.assert_shares(ref[2], f"degree {degree} {scan} thr={thr}")


def test_fixture_wall_edge(fresh_world):
    """The edge of the case this feature exists for: the arm against the wall and everything against the scene FREE, the held box
    against the wall COLLISION, stopped before the crossing."""
    from ca_ref import COLLISION
    x = hca.scene("c1")
    out = hca.wall_edge(x)
    assert out is not None, "no edge carries the box through the wall with the arm clear"
    pts, r, s, g, t_free, cross = out
    ref = hca.edge_reference(x, pts, r, s[None], g[None], hca.MAXD)
    from numbotics_amd.engine import held_edge_shape_motion_bounds
    hm, shapes = hcc.held_robot_model(x.sm, x.spec)
    ht.assert_bits(held_edge_shape_motion_bounds(x.sm, x.spec, s[None], g[None]), edge_shape_motion_bounds(hm, s[None], g[None])[:, shapes],
                   "the wall edge's mu")
    assert ref[3][0] == COLLISION and not ref[0][0] and ref[2][0] == t_free < cross
