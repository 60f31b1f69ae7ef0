"""Inputs and the reference of the held-object tests (tests/test_held_host.py on the CPU, tests/test_gpu_held.py on the GPU).

The reference is the CPU oracle as it is, on ``held_model(sm, spec, G)``: ``sm`` with the held shapes appended as robot shapes
S .. S+H-1 of the holding frame, ``rshape_local`` the NumPy restatement of (A . G) . L_h in xf_mul's operation order
(``locals_ref``), the world references shifted to (S+H)+w, and the pairs (s, S+h) for the allowed robot shapes and (S+h, (S+H)+w)
for the allowed world shapes -- with ``keep_scene`` behind the scene's own.  No test functions here."""
import dataclasses
from fractions import Fraction

import numpy as np

SH_SPHERE, SH_CAPSULE, SH_BOX, SH_CYLINDER = 0, 1, 2, 3
THRESHOLDS = (0.0, 0.01, -0.002)
BATCHES = (1, 63, 64, 65, 1000)
BOX_HALF = (0.1, 0.1, 0.2)          # the parity fixtures' box: margin 0.04, 0.25 m along the gripper's z
BOX_MARGIN = 0.04
BOX_Z = 0.25
PARK = np.array([0.0, 0.0, -6.0])   # where the held bodies' world copies stand: out of every arm's reach


def fma(a, b, c):
    """round(a * b + c) with one rounding, as the hardware's fused multiply-add (exact rational arithmetic, then float())."""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return float(a * b + c)
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def xf_mul_ref(a, b):
    """(3, 4) = a . b for (3, 4) / (4, 4) poses: csrc/nbk_device.hpp xf_mul, operation by operation."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    o = np.zeros((3, 4))
    for i in range(3):
        a0, a1, a2 = a[i, 0], a[i, 1], a[i, 2]
        for j in range(3):
            o[i, j] = fma(a2, b[2, j], fma(a1, b[1, j], float(a0 * b[0, j])))
        o[i, 3] = fma(a2, b[2, 3], fma(a1, b[1, 3], fma(a0, b[0, 3], a[i, 3])))
    return o


def locals_ref(A, G, L):
    """(H, 3, 4): (A . G) . L_h."""
    AG = xf_mul_ref(A, G)
    return np.array([xf_mul_ref(AG, Lh) for Lh in np.asarray(L, dtype=np.float64)]).reshape(-1, 3, 4)


def trans(x, y, z):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def rot_pose(rng, scale=0.3, shift=0.05):
    """A random grasp near BOX_Z along z: a rotation vector of norm <= scale and a translation jitter."""
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(rng.uniform(-scale, scale, 3)).as_matrix()
    T[:3, 3] = np.array([0.0, 0.0, BOX_Z]) + rng.uniform(-shift, shift, 3)
    return T


def held_model(sm, spec, G=None, keep_scene=False, world=True, robot=True):
    """``sm`` with the held shapes of ``spec`` (a HeldSpec, or anything with its fields) as robot shapes.  ``G``: the grasp (default:
    the spec's).  ``world`` / ``robot``: keep only that half of the held pairs."""
    G = spec.G if G is None else G
    S, W, H = sm.n_rshapes, sm.n_wshapes, int(len(spec.shape_type))
    loc = locals_ref(spec.A, G, spec.shape_local).reshape(H, 12)
    pa, pb = [], []
    if robot:
        for s in spec.robot_shapes:
            for h in range(H):
                pa.append(int(s)); pb.append(S + h)
    if world:
        for h in range(H):
            for w in spec.world_shapes:
                pa.append(S + h); pb.append(S + H + int(w))
    pa, pb = np.array(pa, dtype=np.int32), np.array(pb, dtype=np.int32)
    if keep_scene:
        # the arm's own pairs first (NOT sorted: the oracle takes pairs in the order given); their world references move up by H
        pa = np.concatenate((sm.pair_a, pa)).astype(np.int32)
        pb = np.concatenate((np.where(sm.pair_b >= S, sm.pair_b + H, sm.pair_b), pb)).astype(np.int32)
    return dataclasses.replace(
        sm, rshape_frame=np.concatenate((sm.rshape_frame, np.full(H, spec.frame))).astype(np.int32),
        rshape_type=np.concatenate((sm.rshape_type, spec.shape_type)).astype(np.int32),
        rshape_local=np.ascontiguousarray(np.concatenate((sm.rshape_local.reshape(S, 12), loc))),
        rshape_param=np.ascontiguousarray(np.concatenate((sm.rshape_param.reshape(S, 4), np.asarray(spec.shape_param).reshape(H, 4)))),
        rshape_link=np.concatenate((sm.rshape_link, np.zeros(H))).astype(np.int32), pair_a=pa, pair_b=pb)


def held_mask(sm, spec, q, thr, G=None, **kw):
    """The oracle's verdicts of q for the held pairs; all free where there is no pair (the oracle needs one)."""
    from oracle.cpu_oracle import Oracle
    q = np.asarray(q, dtype=np.float64).reshape(-1, sm.kin.n_q)
    m = held_model(sm, spec, G, **kw)
    if m.n_pairs == 0:
        return np.zeros((q.shape[0],), dtype=bool)
    return Oracle(m).validity(q, thr, nthreads=8)


def held_edges_ref(sm, spec, s, g, resolution, max_distance, mode="connect", thr=0.0, dist=None, G=None, **kw):
    from oracle.cpu_oracle import Oracle
    return Oracle(held_model(sm, spec, G, **kw)).edge_validity(s, g, resolution, max_distance, mode=mode, threshold=thr, dist=dist, nthreads=8)


def box(half=BOX_HALF, margin=BOX_MARGIN, **kw):
    """The held box as a PhysicsObject, its world copy parked out of reach."""
    from numbotics_amd.physics import Cuboid
    return Cuboid(0.0, np.array(half, dtype=np.float64), collision_margin=margin, position=PARK.copy(), **kw)


def gripper_box(arm, touch_links=(), **kw):
    """-> (attachment, box): the parity fixtures' box on the ``gripper`` link."""
    b = box(**kw)
    return arm.attach(b, "gripper", pose=trans(0.0, 0.0, BOX_Z), touch_links=touch_links), b


# the robot-pair fixture: a long thin box reaching from the gripper back past the wrist to the forearm, in a scene whose only world
# shape is the box's own parked copy (c1: the arm alone), so the world list is empty and every verdict is a held-robot pair's.  The
# size was tuned with the oracle (tests/test_held_host.py pins the share it decides: at least 5 % of sample_q(chain, 2000, seed=3))
REACH_HALF = (0.03, 0.03, 0.30)
REACH_POSE = trans(0.12, 0.0, -0.20)


def reach_box(arm):
    from numbotics_amd.physics import Cuboid
    b = Cuboid(0.0, np.array(REACH_HALF), collision_margin=0.003, position=PARK.copy())
    return arm.attach(b, "gripper", pose=REACH_POSE), b


def edge_set(q, E, seed=5):
    """E edges a -> a + U(-0.5, 0.5)."""
    rng = np.random.default_rng(seed)
    s = q[:E].copy()
    return s, s + rng.uniform(-0.5, 0.5, s.shape)


def pack_bits(mask):
    from cloud_cases import pack_bits as pb
    return pb(mask)
