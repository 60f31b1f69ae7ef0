"""Shared pieces of the long-chain tests (test_long_chains_host.py on the CPU, test_gpu_long_chains.py on the GPU): the size ladder of
generated robots with 9 to 32 joints, built identically in every process; plain ``np.longdouble`` restatements of FK and of the
Jacobian written from the KinematicModel tables alone (they share no code with the oracle); and a restatement of the LDS byte
formulas by which the library decides whether an entry point serves a descriptor (csrc/nbk.hip ``*_lds()``, csrc/nbk_tables.hpp
``check_limits``).  The point-cloud ladder (tests/cloud_ladder_cases.py) reuses the cases k9, k16, k25, k32d and tree as they are.  No
test functions here."""
import os

import numpy as np

LDS_MAX = 160 * 1024          # bytes of LDS per workgroup
ROW = 512                     # one LDS row: 64 lanes x 8 bytes
BATCHES = (1, 63, 64, 65, 130)
THRESHOLDS = (0.0, 0.01, -0.002)
N_VALIDITY, N_EDGES, N_SPLINES = 4200, 200, 64
N_CERTIFIED = 32              # edges of the certified check that are compared with the NumPy restatement of its loop
N_CERTIFIED_STEER = 16        # ... of the edges again in steer mode at threshold 0.01
N_CERTIFIED_SPLINES = 10      # ... and trajectories (the restatement evaluates every pair at every stop: seconds per trajectory on k32d)
EDGE_RESOLUTION, SPLINE_RESOLUTION = 0.05, 0.05
MAX_DISTANCE = {"connect": 10.0, "steer": 0.6}
SPLINE_CASES = ("k16", "k32d", "tree")
SPLINE_SHAPES = ((3, 6), (5, 8))                # (degree, control points)
IK_CASES = (("k9", None), ("k16", None), ("k24", None), ("k32s", 12))      # (case, path length of the frame; None = the deepest)

# name -> joints, robot shapes, fixed joints (the random_urdf tree: links), seed, gap (self pairs of links fewer than ``gap`` apart
# are removed: dense chains collide with themselves at every configuration otherwise), obstacles.  Seeds and gaps were settled
# with test_long_chains_host.py's input conditions; configurations are drawn over the full joint limits.
CASES = {
    "k9": dict(joints=9, shapes=12, fixed=1, seed=9001, gap=3, obstacles=2),
    "k16": dict(joints=16, shapes=16, fixed=2, seed=16001, gap=6, obstacles=2),
    "k18": dict(joints=18, shapes=17, fixed=0, seed=18001, gap=4, obstacles=2),
    "k24": dict(joints=24, shapes=24, fixed=3, seed=24060, gap=10, obstacles=3),
    "k25": dict(joints=25, shapes=20, fixed=0, seed=25001, gap=6, obstacles=2),
    "k32s": dict(joints=32, shapes=16, fixed=0, seed=32002, gap=5, obstacles=2),
    "k32d": dict(joints=32, shapes=48, fixed=0, seed=32002, gap=16, obstacles=3),
    "tree": dict(links=30, seed=30154, gap=2, obstacles=2),
}
NAMES = tuple(CASES)
# the robot with exact unit axes of the finite-difference check (no table row: kinematics only)
ALIGNED = dict(joints=20, shapes=8, fixed=1, seed=20001)


def fresh():
    from numbotics_amd.physics import World
    from numbotics_amd.physics.world import _reset_worlds
    _reset_worlds()
    World()


def case(name, tmp):
    """-> (arm, chain, obstacles) of ladder case ``name`` in a fresh world; the same in every process."""
    from numbotics_amd.physics import GraphChain
    from numbotics_amd.robots import Arm
    from random_scenes import random_spec_robot, random_urdf, random_obstacles
    p = CASES[name]
    fresh()
    rng = np.random.default_rng(p["seed"])
    path = os.path.join(str(tmp), f"long_chain_{name}.urdf")
    if name == "tree":
        random_urdf(rng, p["links"], path, max_back=3)
    else:
        random_spec_robot(rng, path, n_joints=p["joints"], n_shapes=p["shapes"], axis_mode="mixed", fixed_joints=p["fixed"])
    chain = GraphChain.from_urdf(path)
    arm = Arm(chain)
    obs = random_obstacles(rng, p["obstacles"])
    n_links = len(chain._links)
    for i in range(n_links):
        for j in range(i + 2, min(i + p["gap"], n_links)):
            arm.remove_collision_pair(f"l{i}", f"l{j}")
    return arm, chain, obs


def aligned_robot(tmp):
    """-> (arm, chain) of a 20-joint chain whose revolute axes are exact unit vectors (+-e_x, e_y, e_z)."""
    from numbotics_amd.physics import GraphChain
    from numbotics_amd.robots import Arm
    from random_scenes import random_spec_robot
    fresh()
    rng = np.random.default_rng(ALIGNED["seed"])
    path = random_spec_robot(rng, os.path.join(str(tmp), "long_chain_aligned.urdf"), n_joints=ALIGNED["joints"],
                             n_shapes=ALIGNED["shapes"], axis_mode="aligned", fixed_joints=ALIGNED["fixed"])
    chain = GraphChain.from_urdf(path)
    return Arm(chain), chain


def limits(chain):
    """Joint limits with continuous joints as [-pi, pi]."""
    lim = np.asarray(chain.joint_limits, dtype=np.float64)
    return np.where(np.isfinite(lim), lim, np.sign(lim) * np.pi)


def sample(chain, n, seed):
    lim = limits(chain)
    return np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], (n, chain.dof))


def collision_q(name, chain):
    """The configurations of the validity tests."""
    return sample(chain, N_VALIDITY, 101)


def edges(name, chain):
    """The edges of the edge tests: starts over the joint limits, goals a short way towards another sample."""
    s, g = sample(chain, N_EDGES, 103), sample(chain, N_EDGES, 104)
    step = np.random.default_rng(105).uniform(0.02, 0.25, (N_EDGES, 1))
    return s, s + step * (g - s)


def splines(name, chain, n_ctrl):
    """The control points (N_SPLINES, n_ctrl, dof) of the trajectory tests: short random walks from samples over the joint limits."""
    rng = np.random.default_rng(107 + n_ctrl)
    lim = limits(chain)
    start = rng.uniform(lim[:, 0], lim[:, 1], (N_SPLINES, 1, chain.dof))
    width = rng.uniform(0.004, 0.06, (N_SPLINES, 1, 1))
    steps = rng.uniform(-1.0, 1.0, (N_SPLINES, n_ctrl, chain.dof)) * width * (lim[:, 1] - lim[:, 0])
    steps[:, 0] = 0.0
    return start + np.cumsum(steps, axis=1)


def frames_by_path(kin):
    """{path length: the first link frame, in chain order, with a path of that many joints}."""
    out = {}
    for f in kin.link_names:
        out.setdefault(len(kin.frames[f].path), f)
    return out


def probe_frames(kin):
    """First, middle and last link frame of the chain."""
    names = list(kin.link_names)
    return [names[0], names[len(names) // 2], names[-1]]


def deepest_frame(kin):
    """The link frame with the longest joint path (the last one of these on ties)."""
    return max(kin.link_names, key=lambda f: (len(kin.frames[f].path), kin.link_names.index(f)))


# ---- long-double kinematics from the model tables ---------------------------------------------------------------------------
LD = np.longdouble


def _T44(p12):
    T = np.eye(4, dtype=LD)
    T[:3, :4] = np.asarray(p12, dtype=LD).reshape(3, 4)
    return T


def _joint_motion(kin, k, qk):
    """The 4x4 motion of joint k at value qk in the joint's own frame: the model's rotation a a^T (1 - cos q) + I cos q + [a]x sin q
    with the axis as given (URDF axes carry five digits and are not unit vectors), or a slide along the axis."""
    a = np.asarray(kin.joint_axis[k], dtype=LD)
    X = np.eye(4, dtype=LD)
    if int(kin.joint_type[k]) == 0:
        c, s = np.cos(qk), np.sin(qk)
        ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=LD)
        X[:3, :3] = np.outer(a, a) * (LD(1) - c) + np.eye(3, dtype=LD) * c + ax * s
    else:
        X[:3, 3] = a * qk
    return X


def _sweep(kin, q, frame):
    """World poses of the joint frames along the path of ``frame`` (after each joint's motion) and of the frame itself."""
    fr = kin.frames[frame]
    q = np.asarray(q, dtype=LD)
    T = _T44(kin.base_pose)
    along = []
    for k in fr.path:
        k = int(k)
        T = T @ _T44(kin.joint_offset[k]) @ _joint_motion(kin, k, q[int(kin.joint_qidx[k])])
        along.append(T)
    return along, T @ np.asarray(fr.local, dtype=LD)


def fk_longdouble(kin, q, frame):
    """(4, 4) long-double pose of ``frame`` at one configuration q (n_q,)."""
    return _sweep(kin, q, frame)[1]


def jacobian_longdouble(kin, q, frame):
    """(6, n_q) long-double Jacobian [v; w] of ``frame`` at one configuration: column qidx[k] of a revolute joint k on the path is
    w x (p_end - o_k) over w = R_k a; of a prismatic joint, w over zero."""
    along, E = _sweep(kin, q, frame)
    J = np.zeros((6, kin.n_q), dtype=LD)
    for T, k in zip(along, kin.frames[frame].path):
        k = int(k)
        w = T[:3, :3] @ np.asarray(kin.joint_axis[k], dtype=LD)
        col = int(kin.joint_qidx[k])
        if int(kin.joint_type[k]) == 0:
            J[:3, col] = np.cross(w, E[:3, 3] - T[:3, 3])
            J[3:, col] = w
        else:
            J[:3, col] = w
    return J


# ---- the LDS need of each entry point, restated -----------------------------------------------------------------------------
SHAPE_ROWS = {0: 3, 1: 6, 2: 12, 3: 6, 5: 12}       # LDS rows per robot shape by the model's shape type (sphere, capsule, box, cylinder, hull)
ENTRY_POINTS = ("parked", "distances", "proximity", "ik", "jacobian", "fk_frames", "records")


def frame_slots(kin):
    """Joints whose frame is saved in LDS: those with a child joint other than the next joint."""
    par = np.asarray(kin.joint_parent)
    return len({int(par[k]) for k in range(kin.n_joints) if par[k] >= 0 and par[k] != k - 1})


def shape_rows(sm):
    return int(sum(SHAPE_ROWS[int(t)] for t in sm.rshape_type))


def lds_need(sm, kin, what, path_len=None):
    """Bytes of LDS per workgroup that entry point ``what`` asks for; it serves the descriptor iff this is at most LDS_MAX
    (the all-pairs entry points also need the parked layout).  ``sm`` may be None for the kinematic entry points."""
    n_q, J, slots = kin.n_q, kin.n_joints, frame_slots(kin)
    if what == "ik":
        return ROW * (7 * n_q + 6 * max(int(path_len), 1))
    if what == "jacobian":
        return ROW * (7 * n_q + 1)
    if what == "fk_frames":
        return ROW * max(n_q, 17) + ROW * (n_q + 12 * slots)
    if what == "records":                               # item records with gradient rows: nothing is parked
        return ROW * (max(n_q, 1) + 6 * J)
    parked = ROW * (n_q + max(shape_rows(sm), n_q) + 12 * slots) + 2304
    if what == "parked":
        return parked
    if what == "distances":
        return parked + 1536
    if what == "proximity":
        return parked + 1536 + ROW * 6 * J
    raise ValueError(what)


def served(sm, kin, what, path_len=None):
    """The restated verdict.  ``closest`` needs the parked layout alone; ``pair_distances`` and ``proximity_jacobian`` need it too."""
    if what in ("distances", "proximity") and lds_need(sm, kin, "parked") > LDS_MAX:
        return False
    return lds_need(sm, kin, what, path_len) <= LDS_MAX


def ik_frame(kin, path_len):
    return deepest_frame(kin) if path_len is None else frames_by_path(kin)[path_len]


def ik_problems(orc, chain, frame, n, seed=109):
    """Targets from FK of random configurations over the full limits, starts within +-0.1 of them -> (pose (n, 4, 4), q0 (n, dof))."""
    qt = sample(chain, n, seed)
    q0 = qt + np.random.default_rng(seed + 1).uniform(-0.1, 0.1, qt.shape)
    return orc.fk(qt, frame), q0
