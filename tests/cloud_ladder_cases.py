"""Shared inputs of the point-cloud tests on the long-chain ladder (test_cloud_ladder_host.py on the CPU, test_gpu_cloud_ladder.py
on the GPU): the robots, their configurations, edges, clouds and shape selections, built identically in every process.  No test
functions here.

Robots: k9, k16, k25, k32d and tree of tests/long_chain_cases.py as they are, and ``s72``: a serial chain of 32 joints and 72 robot
shapes (up to three per link, some links empty) whose shapes are handed to the library in a SHUFFLED order.  An arm compiled from a
URDF lists its shapes link by link in topological order, which on a serial chain is the library's device (frame) order already; a
descriptor may list them in any order, and only then do the caller's index (the selection's bits, the clearance's reported shape,
the motion bound's column) and the device index (the walk, the selection words the kernels read) differ.  72 shapes need two
selection words.

Clouds: no scan of a wall and a table (placed for a 0.9 m arm) but points near where the robot's shapes pass: centres of robot
shapes at some of the test's own configurations and at interior points of some of its edges, displaced by 0 .. ``hi`` metres in a
random direction (0: inside the shape's core, which is what sends a box or a cylinder to EPA), and taken only where few of the
configurations come near (``points``: a long chain coils around its base, and a point placed anywhere near it collides in almost
every row; one next to a shape of the base frame, which never moves, in every row or in none).  At most 300 points."""
import dataclasses
import functools
import tempfile

import numpy as np

import long_chain_cases as L
from cloud_cases import cloud_mask, cloud_closest

ROBOTS = ("k9", "k16", "k25", "k32d", "tree", "s72")
B_MAX = 130
BATCHES = (1, 63, 64, 65, 130)
THRESHOLDS = (0.0, 0.02, -0.005)
RADII = (0.01, 0.0)
D_MAX = (0.02, 0.5)
E_SIZES = (1, 63, 65, 130)
RESOLUTION, MAXD = 0.02, 0.15          # sampled edges
STEER_MAXD = 0.15                      # certified edges in steer mode (connect: 10.0)
INF = float("inf")
# (mode, dist given, look_ahead, shapes) -- test_gpu_cloud_continuous.CONFIGS
CONFIGS = [("connect", False, 0.03, "arm"), ("steer", False, INF, "arm"), ("steer", True, 0.03, "sub"), ("connect", True, INF, "sub")]

# s72: 32 joints hold 72 shapes at up to three per link.  lds_broad_ok (csrc/nbk_lds.hpp) accepts a serial chain (no saved frame slots)
# with 512 n_q + 1536 S + 32 P + 144 W + 2048 <= 163840 bytes: at n_q = 32, S = 72 that leaves room for 1088 pairs without world
# shapes.  gap = 30 keeps the self pairs of links 30 or more apart (P = 96 with the one obstacle's pairs); the cloud entries ignore them.
S72 = dict(joints=32, shapes=72, fixed=0, seed=72001, gap=30, obstacles=1, shuffle=72002)

# name -> the clouds' parameters, settled on the CPU with the oracle alone (test_cloud_ladder_host.py asserts the conditions; ``points``
# says what each does): the values are the first tried that met every condition on all six robots, then length was shortened from 0.5
# where more than a quarter of the certified edges ran out of iterations (the motion bound of a long chain is large).  hi: largest
# displacement from a shape centre; mids / mid_share: edges that lend interior configurations, and the share of candidates drawn there;
# most / cover / free: the filter; length: longest edge in joint space; focus / weight (s72): shapes drawn more often, so that straddle
# and high meet enough points; one_high (s72): a shape >= 64 the reference shows colliding (in 0.17 of the rows).
CLOUDS = {
    "k9": dict(seed=9, hi=0.07, mids=30, mid_share=0.3, most=2, cover=0.4, free=80, length=0.4),
    "k16": dict(seed=16, hi=0.07, mids=30, mid_share=0.3, most=2, cover=0.4, free=80, length=0.25),
    "k25": dict(seed=25, hi=0.07, mids=30, mid_share=0.3, most=2, cover=0.4, free=80, length=0.25),
    "k32d": dict(seed=32, hi=0.07, mids=30, mid_share=0.3, most=2, cover=0.4, free=80, length=0.25),
    "tree": dict(seed=30, hi=0.10, mids=30, mid_share=0.3, most=2, cover=0.4, free=80, length=0.25),
    "s72": dict(seed=72, hi=0.07, mids=30, mid_share=0.3, most=2, cover=0.4, free=80, length=0.25, focus=(62, 63, 64, 65, 66, 67, 68, 69, 70, 71),
                weight=4.0, one_high=67),
}
N_POINTS = 300
E_CASE = {"k9": 34, "k16": 34, "k25": 34, "k32d": 34, "tree": 34, "s72": 34}      # certified edges compared (the last two degenerate)


@dataclasses.dataclass
class Robot:
    name: str
    sm: object            # SceneModel (s72: with its robot shapes shuffled)
    limits: np.ndarray    # (dof, 2)
    q: np.ndarray         # (B_MAX, dof)
    keep: tuple           # what the scene model's links and objects belong to


def shuffle_shapes(sm, perm):
    """``sm`` with robot shape j = shape perm[j] of before; the pairs follow (robot-robot pairs smaller index first, sorted as
    SceneModel sorts them)."""
    S = sm.n_rshapes
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty(S, dtype=np.int64)
    inv[perm] = np.arange(S)
    pa = inv[sm.pair_a]
    pb = np.where(sm.pair_b < S, inv[np.minimum(sm.pair_b, S - 1)], sm.pair_b)
    lo, hi = np.where(pb < S, np.minimum(pa, pb), pa), np.where(pb < S, np.maximum(pa, pb), pb)
    order = np.lexsort((hi, lo))
    return dataclasses.replace(sm, rshape_frame=np.ascontiguousarray(sm.rshape_frame[perm]), rshape_type=np.ascontiguousarray(sm.rshape_type[perm]),
                               rshape_local=np.ascontiguousarray(sm.rshape_local[perm]), rshape_param=np.ascontiguousarray(sm.rshape_param[perm]),
                               rshape_link=np.ascontiguousarray(sm.rshape_link[perm]), pair_a=lo[order].astype(np.int32),
                               pair_b=hi[order].astype(np.int32))


def _s72(tmp):
    import os
    from numbotics_amd.physics import GraphChain
    from numbotics_amd.robots import Arm
    from random_scenes import random_spec_robot, random_obstacles
    p = S72
    L.fresh()
    rng = np.random.default_rng(p["seed"])
    path = os.path.join(str(tmp), "cloud_ladder_s72.urdf")
    random_spec_robot(rng, path, n_joints=p["joints"], n_shapes=p["shapes"], axis_mode="mixed", fixed_joints=p["fixed"])
    chain = GraphChain.from_urdf(path)
    arm = Arm(chain)
    obs = random_obstacles(rng, p["obstacles"])
    n_links = len(chain._links)
    for i in range(n_links):
        for j in range(i + 2, min(i + p["gap"], n_links)):
            arm.remove_collision_pair(f"l{i}", f"l{j}")
    sm = arm.scene_model()
    perm = np.random.default_rng(p["shuffle"]).permutation(sm.n_rshapes)
    # a shape of the last joint's frame goes to position 70: joint 31 is then on a path under ``high``, whose bits lie in word 1
    j = int(np.flatnonzero(sm.rshape_frame[perm] == sm.kin.n_joints - 1)[0])
    perm[[j, 70]] = perm[[70, j]]
    return arm, chain, obs, shuffle_shapes(sm, perm)


@functools.lru_cache(maxsize=None)
def robot(name):
    """The ladder robot ``name``, built once per process (its scene model is plain arrays: it outlives the world it was built in)."""
    with tempfile.TemporaryDirectory() as tmp:
        if name == "s72":
            arm, chain, obs, sm = _s72(tmp)
        else:
            arm, chain, obs = L.case(name, tmp)
            sm = arm.scene_model()
    return Robot(name, sm, L.limits(chain), L.sample(chain, B_MAX, 211), (arm, chain, obs))


def device_order(sm):
    """Descriptor index of the robot shape at each device position: csrc/nbk_tables.hpp order_shapes restated -- the shapes of frame
    -1 (the base), then of joint frame 0, 1, ..., each group in the caller's order (a stable sort by frame).  No host-only entry of the
    library hands its own table out."""
    return np.argsort(np.asarray(sm.rshape_frame), kind="stable")


def lds_broad_bytes(sm):
    """What lds_broad_ok (csrc/nbk_lds.hpp) compares with LDS_MAX = 163840: the LDS broadphase's layout with the q slab as n_q rows and
    the queue counted on top; nbk_model_create refuses a robot of more than 16 shapes beyond it."""
    return (L.ROW * sm.kin.n_q + L.ROW * 12 * L.frame_slots(sm.kin) + L.ROW * 3 * sm.n_rshapes + 32 * sm.n_pairs + 144 * sm.n_wshapes
            + 2048)


def selections(rb):
    """The shape selections of a robot, in the caller's numbering."""
    sm, S = rb.sm, rb.sm.n_rshapes
    out = {"all": None, "arm": [s for s in range(S) if sm.rshape_frame[s] >= 0], "sub": [S - 3, S - 2, S - 1]}
    if rb.name == "s72":
        out.update(straddle=[62, 63, 64, 65, S - 1], high=list(range(64, S)), low=list(range(64)), one_high=[CLOUDS["s72"]["one_high"]])
    return out


def edges(rb):
    """130 edges: starts at the configurations, goals 0.02 .. ``length`` away in a random direction."""
    rng = np.random.default_rng(7)
    s = rb.q.copy()
    d = rng.standard_normal(s.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return s, s + d * rng.uniform(0.02, CLOUDS[rb.name]["length"], (s.shape[0], 1))


def certified_edges(rb, E=None):
    """E edges (default E_CASE): the first E - 2 edges and two degenerate ones."""
    s, g = edges(rb)
    n = (E_CASE[rb.name] if E is None else E) - 2
    return np.concatenate((s[:n], s[:2])), np.concatenate((g[:n], s[:2] + 1e-9))


def given_dist(s, g):
    return 1.1 * np.linalg.norm(g - s, axis=1)


def _T44(p12):
    T = np.eye(4)
    T[:3, :4] = np.asarray(p12, dtype=np.float64).reshape(3, 4)
    return T


def shape_centres(sm, q, shapes):
    """(len(q), len(shapes), 3) world centres of the robot shapes at q, by the oracle's FK of each shape's link."""
    from oracle.cpu_oracle import Oracle
    orc = Oracle(sm.kin)
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, sm.kin.n_q)
    out = np.empty((q.shape[0], len(shapes), 3))
    poses = {}
    for k, s in enumerate(shapes):
        link = sm.links[sm.rshape_link[s]]._name
        if link not in poses:
            poses[link] = orc.fk(q, link) @ np.linalg.inv(np.asarray(sm.kin.frames[link].local, dtype=np.float64))
        out[:, k] = (poses[link] @ _T44(sm.rshape_local[s]))[:, :3, 3]
    return out


def bound_radii(sm, shapes):
    """Radius of the ball about each shape's centre that holds the shape: its core's bounding radius plus its margin, as
    csrc/nbk_tables.hpp motion_tables takes it (sphere, capsule, box, cylinder; the ladder has no hulls)."""
    p = np.asarray(sm.rshape_param, dtype=np.float64)
    m = p[:, 3]                                   # the margin of a box or a cylinder: its core is that much smaller
    by_type = {0: p[:, 0], 1: p[:, 0] + p[:, 1], 2: np.linalg.norm(p[:, :3] - m[:, None], axis=1) + m, 3: np.hypot(p[:, 0] - m, p[:, 1] - m) + m}
    return np.array([by_type[int(sm.rshape_type[s])][s] for s in shapes])


@functools.lru_cache(maxsize=None)
def points(name, which="arm", seed_shift=0):
    """The cloud ``which`` ("arm": for the selections None, arm and those of s72; "sub": for the last three shapes) of a robot, (N, 3)
    with N <= 300, two of them duplicates of earlier points (ties of the clearance go to the smaller index).

    Candidates are centres of the cloud's shapes (the ``focus`` shapes ``weight`` times as often) at the 130 configurations and at
    interior points of ``mids`` edges, displaced by up to ``hi``.  A long chain is a coil around its base: a point anywhere near it is
    touched at most configurations by SOME shape.  So a candidate is taken only if the balls about the shape centres (bound radius +
    0.045: the largest threshold, the radius and a margin) hold it at no more than ``most`` configurations, and only while the
    configurations so touched by the cloud stay below ``cover`` of the 130; at most ``free`` points that no configuration touches
    (they lie on edges) are taken."""
    rb = robot(name)
    sm, c = rb.sm, CLOUDS[name]
    sel = selections(rb)
    looked_at = list(range(sm.n_rshapes)) if which == "arm" else sel["sub"]
    src = [s_ for s_ in (sel["arm"] if which == "arm" else sel["sub"]) if sm.rshape_frame[s_] >= 0]
    w = np.array([c.get("weight", 1.0) if s_ in c.get("focus", ()) else 1.0 for s_ in src])
    rng = np.random.default_rng(1000 * c["seed"] + (0 if which == "arm" else 1) + 17 * seed_shift)
    s, g = edges(rb)
    mids = rng.choice(B_MAX, c["mids"], replace=False)
    f = rng.uniform(0.3, 0.9, (c["mids"], 1))
    at = np.concatenate((rb.q, s[mids] + f * (g[mids] - s[mids])))
    centres = shape_centres(sm, at, src)
    n_cand = 6000
    d = rng.standard_normal((n_cand, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    from_mid = rng.random(n_cand) < c["mid_share"]
    ci = np.where(from_mid, B_MAX + rng.integers(0, c["mids"], n_cand), rng.integers(0, B_MAX, n_cand))
    cand = centres[ci, rng.choice(len(src), n_cand, p=w / w.sum())] + d * rng.uniform(0.0, c["hi"], (n_cand, 1))
    cen = shape_centres(sm, rb.q, looked_at)
    reach = bound_radii(sm, looked_at) + 0.045
    near = np.zeros((B_MAX, n_cand), dtype=bool)
    for k in range(len(looked_at)):
        near |= np.linalg.norm(cen[:, k, None, :] - cand[None], axis=2) < reach[k]
    count = near.sum(axis=0)
    covered = np.zeros(B_MAX, dtype=bool)
    picked, n_free = [], 0
    for n in range(n_cand):
        if count[n] > c["most"] or (count[n] == 0 and n_free >= c["free"]):
            continue
        if (covered | near[:, n]).sum() > c["cover"] * B_MAX:
            continue
        covered |= near[:, n]
        n_free += count[n] == 0
        picked.append(n)
        if len(picked) == N_POINTS:
            break
    pts = cand[picked]
    N = pts.shape[0]
    pts[N - 1] = pts[7]
    pts[N // 2] = pts[N // 2 + 50]
    pts = np.ascontiguousarray(pts)
    pts.setflags(write=False)
    return pts


def bounds(name):
    """A box that holds every cloud of the robot (the graph test swaps points under one grid)."""
    p = np.concatenate([points(name, w, k) for w in ("arm", "sub") for k in (0, 1)])
    return (p.min(0) - 0.05).tolist(), (p.max(0) + 0.05).tolist()


def _key(shapes):
    return None if shapes is None else tuple(shapes)


@functools.lru_cache(maxsize=None)
def _mask(name, which, seed_shift, r, thr, shapes):
    rb = robot(name)
    out = cloud_mask(rb.sm, points(name, which, seed_shift), r, rb.q, thr, None if shapes is None else list(shapes))
    out.setflags(write=False)
    return out


def mask_ref(name, which, r, thr, shapes, seed_shift=0):
    """The oracle's verdicts of the robot's 130 configurations (computed once per process)."""
    return _mask(name, which, seed_shift, r, thr, _key(shapes))


@functools.lru_cache(maxsize=None)
def _closest(name, which, seed_shift, r, d_max, shapes):
    rb = robot(name)
    out = cloud_closest(rb.sm, points(name, which, seed_shift), r, rb.q, d_max, None if shapes is None else list(shapes))
    for a in out:
        a.setflags(write=False)
    return out


def closest_ref(name, which, r, d_max, shapes, seed_shift=0):
    return _closest(name, which, seed_shift, r, d_max, _key(shapes))


@functools.lru_cache(maxsize=None)
def _sampled(name, which, seed_shift, r, thr, mode, given, shapes):
    from oracle.cpu_oracle import Oracle
    from cloud_cases import cloud_model
    rb = robot(name)
    s, g = edges(rb)
    dist = given_dist(s, g) if given else None
    return Oracle(cloud_model(rb.sm, points(name, which, seed_shift), r, None if shapes is None else list(shapes))).edge_validity(
        s, g, RESOLUTION, MAXD, mode=mode, threshold=thr, dist=dist, nthreads=8)


def sampled_ref(name, which, r, thr, mode, given, shapes, seed_shift=0):
    """The oracle's (valid, end, n_samples) of the 130 edges against the cloud."""
    return _sampled(name, which, seed_shift, r, thr, mode, given, _key(shapes))


@functools.lru_cache(maxsize=None)
def _certified(name, which, seed_shift, config, shapes, n):
    from cloud_continuous_ref import reference_cloud_continuous
    rb = robot(name)
    mode, given, la, _ = CONFIGS[config]
    s, g = certified_edges(rb, n)
    dist = given_dist(s, g) if given else None
    return reference_cloud_continuous(rb.sm, points(name, which, seed_shift), RADII[0], s, g, STEER_MAXD if mode == "steer" else 10.0, mode=mode,
                                      threshold=0.0, look_ahead=la, dist=dist, shapes=None if shapes is None else list(shapes))


def certified_ref(name, which, config, shapes, n=None, seed_shift=0):
    """cloud_continuous_ref.reference_cloud_continuous of certified_edges(rb, n) under CONFIGS[config] (its mode, dist and
    look_ahead; ``shapes`` as given)."""
    return _certified(name, which, seed_shift, config, _key(shapes), n)


# ---- the accumulate forms on k16: its own scene (two obstacles and the self pairs the ladder keeps) first, then the cloud ------------
@functools.lru_cache(maxsize=None)
def sampled_accumulate_ref(mode):
    """(the scene alone, the cloud alone, the oracle on the descriptor that holds both) of k16's 130 edges, selection arm."""
    from oracle.cpu_oracle import Oracle
    from cloud_cases import cloud_model
    rb = robot("k16")
    s, g = edges(rb)
    shapes = selections(rb)["arm"]
    own = Oracle(rb.sm).edge_validity(s, g, RESOLUTION, MAXD, mode=mode, threshold=0.0, nthreads=8)
    both = Oracle(cloud_model(rb.sm, points("k16"), RADII[0], shapes, keep_scene=True)).edge_validity(s, g, RESOLUTION, MAXD, mode=mode,
                                                                                                  threshold=0.0, nthreads=8)
    return own, sampled_ref("k16", "arm", RADII[0], 0.0, mode, False, shapes), both


@functools.lru_cache(maxsize=None)
def certified_accumulate_ref(mode, look_ahead):
    """(the scene alone, the cloud alone, one call over scene and cloud) of k16's certified edges, selection arm."""
    from oracle.cpu_oracle import Oracle
    from continuous_ref import reference_continuous
    from cloud_continuous_ref import reference_cloud_continuous
    rb = robot("k16")
    s, g = certified_edges(rb)
    shapes = selections(rb)["arm"]
    maxd = STEER_MAXD if mode == "steer" else 10.0
    orc = Oracle(rb.sm)
    own = reference_continuous(rb.sm, orc, s, g, maxd, mode=mode)
    only = reference_cloud_continuous(rb.sm, points("k16"), RADII[0], s, g, maxd, mode=mode, look_ahead=look_ahead, shapes=shapes)
    both = reference_cloud_continuous(rb.sm, points("k16"), RADII[0], s, g, maxd, mode=mode, look_ahead=look_ahead, shapes=shapes, scene_orc=orc)
    return own, only, both
