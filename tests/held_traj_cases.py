"""Inputs and references of the held-object trajectory tests (tests/test_held_traj_host.py on the CPU, tests/test_gpu_held_traj.py on
the GPU): item distances, certified edges, certified and sampled splines with the object in the hand.

The reference is the CPU oracle and the NumPy restatements of the certified loops as they are, on ``held_cases.held_model``: the
scene's model with the held shapes appended as robot shapes of the holding frame and the held pairs as its pair list (with
``keep_scene`` behind the scene's own).  No test functions here."""
import functools
import types

import numpy as np

import held_cases as hc

MAXD = 10.0                         # max_distance of the edge sets: no edge is cut short in connect mode
MAXD_STEER = 0.6
EDGE_COUNTS = (1, 63, 64, 65, 130)
SPLINE_COUNTS = (1, 64, 65)
BATCHES = (1, 63, 64, 65, 1000)
RESOLUTION = 0.05
N_EDGES, N_SPLINES, N_CTRL = 130, 65, 6
SPREAD = {1: 0.12, 2: 0.12, 3: 0.12, 4: 0.12, 5: 0.12}      # per degree: the spread of the control points about the first


def scene(name):
    """-> namespace(arm, chain, keep, sm, att, spec, q (2000, dof)): ``c3`` with the parity fixtures' box on the gripper, ``c2`` (one
    cube) and ``c1`` (robot pairs only) with the reach box, ``tree`` with a box on tip_b, below two prismatic joints."""
    from numbotics_amd.scenes import build_scene, sample_q
    if name == "tree":
        from continuous_ref import tree_scene, random_edges
        from numbotics_amd.physics import Cuboid
        arm, chain, obs = tree_scene()
        b = Cuboid(0.0, np.array([0.02, 0.03, 0.05]), collision_margin=0.004, position=hc.PARK.copy())
        att = arm.attach(b, "tip_b", pose=hc.trans(0.0, 0.01, 0.06))
        q = random_edges(chain, 2000, 3)[0]
    else:
        arm, chain, obs = build_scene(name)
        # c2 carries the reach box as well: with the gripper box its certified edges are 111 FREE / 13 COLLISION / 6 UNDECIDED of 130
        # by the reference, and 6 misses the 5 % every kind must have; with the reach box they are 75 / 41 / 14, decided by robot
        # items and by the cube
        att, b = hc.gripper_box(arm) if name == "c3" else hc.reach_box(arm)
        q = sample_q(chain, 2000, seed=3)
    return types.SimpleNamespace(arm=arm, chain=chain, keep=(obs, b), sm=arm.scene_model(), att=att, spec=att.spec(arm), q=q)


def edges(x, E=N_EDGES):
    if x.chain.dof != 7:
        from continuous_ref import random_edges
        return random_edges(x.chain, E, 5, scale=0.25)
    return hc.edge_set(x.q, E)


def splines(x, degree=3, S=N_SPLINES, n=N_CTRL):
    """-> ctrl (S, n, dof), knots: the first control point a sampled configuration, the others a random walk from it."""
    from numbotics_amd.planning import unit_knots
    step = np.random.default_rng(7).uniform(-SPREAD[degree], SPREAD[degree], (S, n, x.chain.dof))
    return x.q[:S, None, :] + np.cumsum(step, axis=1), unit_knots(n, degree)


def item_columns(sm, spec):
    """(K, 3) int: (held shape, 0 robot / 1 world, index) of the items, in ``held_model``'s pair order."""
    H = int(len(spec.shape_type))
    out = [(h, 0, int(s)) for s in spec.robot_shapes for h in range(H)]
    out += [(h, 1, int(w)) for h in range(H) for w in spec.world_shapes]
    return np.array(out, dtype=np.int32).reshape(-1, 3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _shared(f):
    """A reference is computed once per (fixture name, arguments) and shared among the tests: ``x``, the scene of that name as the
    caller built it, is only used by the call that computes."""
    memo = {}

    @functools.wraps(f)
    def g(x, *key):
        if key not in memo:
            memo[key] = f(x, *key)
        return memo[key]
    return g


def assert_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if ref.dtype == np.float64:
        bad = bits(got) != bits(ref)
    else:
        bad = got != ref
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[:4].tolist()}: " \
                          f"{got[bad][:4]} != {ref[bad][:4]}"


@_shared
def _edge_ref(x, name, keep_scene, mode, thr, max_iter, E):
    """The certified reference of the first E edges of ``name``: computed once per argument set and shared."""
    from oracle.cpu_oracle import Oracle
    from continuous_ref import reference_continuous
    hm = hc.held_model(x.sm, x.spec, keep_scene=keep_scene)
    s, g = edges(x)
    maxd = MAXD if mode == "connect" else MAXD_STEER
    return reference_continuous(hm, Oracle(hm), s[:E], g[:E], maxd, mode=mode, threshold=thr, max_iter=max_iter)[:4]


def edge_ref(x, name, keep_scene=False, mode="connect", thr=0.0, max_iter=64, E=N_EDGES):
    """valid, end, t_free, status of the first E edges: per-edge results do not depend on E, so the full set is computed once."""
    v, end, t, st = _edge_ref(x, name, bool(keep_scene), mode, float(thr), int(max_iter), N_EDGES)
    return v[:E], end[:E], t[:E], st[:E]


@_shared
def _spline_ref(x, name, keep_scene, degree, thr):
    from oracle.cpu_oracle import Oracle
    from spline_continuous_ref import reference_spline_continuous
    hm = hc.held_model(x.sm, x.spec, keep_scene=keep_scene)
    ctrl, knots = splines(x, degree)
    return reference_spline_continuous(hm, Oracle(hm), ctrl, knots, degree, threshold=thr)[:3]


def spline_ref(x, name, keep_scene=False, degree=3, thr=0.0, S=N_SPLINES):
    v, t, st = _spline_ref(x, name, bool(keep_scene), int(degree), float(thr))
    return v[:S], t[:S], st[:S]


@_shared
def _sampled_ref(x, name, keep_scene, degree, thr):
    from oracle.cpu_oracle import Oracle
    from spline_ref import reference_splines
    ctrl, knots = splines(x, degree)
    return reference_splines(Oracle(hc.held_model(x.sm, x.spec, keep_scene=keep_scene)), ctrl, knots, degree, RESOLUTION, thr)


def sampled_ref(x, name, keep_scene=False, degree=3, thr=0.0, S=N_SPLINES):
    v, t, ns = _sampled_ref(x, name, bool(keep_scene), int(degree), float(thr))
    return v[:S], t[:S], ns[:S]


def shares(status):
    """(FREE, COLLISION, UNDECIDED) counts of a certified status array."""
    from ca_ref import FREE, COLLISION, UNDECIDED
    status = np.asarray(status)
    return int((status == FREE).sum()), int((status == COLLISION).sum()), int((status == UNDECIDED).sum())
