"""NumPy + CPU-oracle restatement of nbk_edge_continuous_batch (ContinuousConnector's device path), for the tests.

Conservative advancement per (edge, pair) item: mu from nbk_edge_motion_bounds_host, distances from ``Oracle.pair_distances``
(the bits the device computes), q(t) = (1 - t) * s + t * g with three roundings; the loop of include/nbk.h and the per-edge
reduction are those of tests/ca_ref.py.  The oracle runs in a few threads (ctypes releases the GIL)."""
import math
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

from numbotics_amd.engine import edge_motion_bounds
from ca_ref import advance_items, reduce_items, FREE, COLLISION, UNDECIDED, DEGENERATE      # noqa: F401  (the codes: for the tests)

F32_EPS = 1.1920928955078125e-07
DBL_MAX = 1.7976931348623157e308


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def edge_span(s, g, dist, max_distance, mode):
    """(d, T_f) of one edge, or None for the degenerate edge -- nbk_edge_validity_batch's rules (fma-accumulated norm)."""
    if dist is None:
        acc = 0.0
        for i in range(s.shape[0]):
            df = float(g[i] - s[i])
            acc = _fma(df, df, acc)
        d = math.sqrt(acc)
    else:
        d = float(dist)
    if not (d > F32_EPS and d <= DBL_MAX):
        return None
    Tf = max_distance / d if (mode == "steer" and d > max_distance) else 1.0
    return d, Tf


def pair_distances(orc, q, threads=8):
    if q.shape[0] < 512:
        return orc.pair_distances(q)
    chunks = np.array_split(q, threads)
    with ThreadPoolExecutor(threads) as ex:
        return np.concatenate(list(ex.map(orc.pair_distances, chunks)), axis=0)


def edge_ends(starts, goals, Tf, live, mode):
    """end (E, n_q): the goal, or q(T_f) in three roundings under "steer"; NaN rows where not ``live``."""
    end = np.full(starts.shape, np.nan)
    for e in np.nonzero(live)[0]:
        end[e] = goals[e] if mode == "connect" else (1.0 - Tf[e]) * starts[e] + Tf[e] * goals[e]
    return end


def reference_continuous(sm, orc, starts, goals, max_distance, mode="connect", threshold=0.0, max_iter=64, slack=1e-6, dist=None):
    """-> valid (E,) bool, end (E, n_q), t_free (E,), status (E,) int32, and the per-item stop points / statuses (E, P)."""
    starts = np.ascontiguousarray(starts, dtype=np.float64)
    goals = np.ascontiguousarray(goals, dtype=np.float64)
    E = starts.shape[0]
    P = sm.n_pairs
    mu = edge_motion_bounds(sm, starts, goals) if P > 0 else np.zeros((E, 0))
    spans = [edge_span(starts[e], goals[e], None if dist is None else dist[e], max_distance, mode) for e in range(E)]
    Tf = np.array([sp[1] if sp is not None else np.nan for sp in spans])
    live = np.array([sp is not None for sp in spans], dtype=bool)

    def distance(ee, pp, tt):
        q = (1.0 - tt)[:, None] * starts[ee] + tt[:, None] * goals[ee]
        return pair_distances(orc, q)[np.arange(ee.shape[0]), pp]
    stop, st = advance_items(distance, mu, Tf, live, threshold, max_iter, slack)
    valid, t_free, status = reduce_items(stop, st, Tf, live)
    end = edge_ends(starts, goals, Tf, live, mode)
    return valid, end, t_free, status, stop, st


def motion_bounds_numpy(sm, starts, goals):
    """mu (E, P) built independently from the model arrays (float64 NumPy, its own summation order)."""
    kin = sm.kin
    J = kin.n_joints
    parent = np.asarray(kin.joint_parent)
    jtype = np.asarray(kin.joint_type)
    qidx = np.asarray(kin.joint_qidx)
    trans = np.asarray(kin.joint_trans, dtype=np.float64).reshape(J, 3)
    slide = np.asarray(kin.joint_slide, dtype=np.float64).reshape(J, 3)

    def path(f):
        out = []
        while f >= 0:
            out.append(int(f))
            f = parent[f]
        return out[::-1]

    S = sm.n_rshapes
    bound = np.empty(S)
    loc = np.empty(S)
    for x in range(S):
        L = np.asarray(sm.rshape_local[x], dtype=np.float64).reshape(-1)
        loc[x] = np.linalg.norm(L[[3, 7, 11]])
        typ, prm = int(sm.rshape_type[x]), np.asarray(sm.rshape_param[x], dtype=np.float64)
        margin = prm[3]
        if typ == 0:        # sphere: a point core inflated by its radius
            rho, margin = 0.0, prm[0]
        elif typ == 1:      # capsule: segment of half length hl
            rho, margin = prm[1], prm[0]
        elif typ == 2:      # box: the core is the box shrunk by the margin
            rho = np.linalg.norm(prm[:3] - margin)
        elif typ == 3:      # cylinder
            rho = math.hypot(prm[0] - margin, prm[1] - margin)
        else:               # hull: largest vertex norm
            h = int(prm[0])
            v = np.asarray(sm.hull_verts, dtype=np.float64).reshape(-1, 3)[sm.hull_vert_begin[h]:sm.hull_vert_begin[h + 1]]
            rho = np.linalg.norm(v, axis=1).max()
        bound[x] = rho + margin
    starts = np.asarray(starts, dtype=np.float64)
    goals = np.asarray(goals, dtype=np.float64)
    mu = np.zeros((starts.shape[0], sm.n_pairs))
    for e in range(starts.shape[0]):
        s, g = starts[e], goals[e]
        dq = np.abs(g - s)
        qmax = np.maximum(np.abs(s), np.abs(g))
        for p in range(sm.n_pairs):
            a, b = int(sm.pair_a[p]), int(sm.pair_b[p])
            pa = path(int(sm.rshape_frame[a]))
            pb = path(int(sm.rshape_frame[b])) if b < S else []
            total = 0.0
            for x, own, other in ((a, pa, pb), (b, pb, pa)):
                for i, j in enumerate(own):
                    if j in other:
                        continue
                    if jtype[j] == 1:
                        c = np.linalg.norm(slide[j])
                    else:
                        below = own[i + 1:]
                        c = sum(np.linalg.norm(trans[k]) for k in below)
                        c += sum(np.linalg.norm(slide[k]) * qmax[qidx[k]] for k in below if jtype[k] == 1)
                        c += loc[x] + bound[x]
                    total += c * dq[qidx[j]]
            mu[e, p] = total
    return mu


TREE_URDF = __import__("os").path.join(__import__("os").path.dirname(__file__), "models", "tree_gripper.urdf")


def tree_scene():
    """tests/models/tree_gripper.urdf (prismatic joints below revolute ones) among four obstacles."""
    from numbotics_amd.physics import GraphChain, Cube, Sphere, Plane, Capsule
    from numbotics_amd.robots import Arm
    chain = GraphChain.from_urdf(TREE_URDF)
    arm = Arm(chain)
    obs = [Cube(0.0, 0.08, position=np.array([0.35, 0.0, 0.55])), Sphere(0.0, 0.05, position=np.array([0.2, 0.2, 0.4])),
           Plane(0.0, np.array([0.0, 0.0, 1.0]), position=np.array([0.0, 0.0, -0.01])),
           Capsule(0.0, 0.03, 0.3, position=np.array([-0.2, 0.1, 0.6]))]
    arm.remove_collision_pair("base", obs[2].name)
    return arm, chain, obs


def random_scene(seed, tmp_path):
    """A random_urdf mechanism among random obstacles; None when it has no joints or no pairs."""
    from numbotics_amd.physics import GraphChain
    from numbotics_amd.robots import Arm
    from random_scenes import random_urdf, random_obstacles
    rng = np.random.default_rng(seed)
    chain = GraphChain.from_urdf(random_urdf(rng, int(rng.integers(4, 9)), str(tmp_path / f"ca_{seed}.urdf")))
    if chain.dof == 0:
        return None
    arm = Arm(chain)
    obs = random_obstacles(rng, int(rng.integers(2, 6)))
    if arm.scene_model().n_pairs == 0:
        return None
    return arm, chain, obs


def random_edges(chain, n, seed, scale=None):
    """n edges between joint-limit samples; ``scale`` shortens them (goal = s + scale (g - s))."""
    rng = np.random.default_rng(seed)
    lim = np.asarray(chain.joint_limits, dtype=np.float64)
    lim = np.where(np.isfinite(lim), lim, np.sign(lim) * np.pi)
    s = rng.uniform(lim[:, 0], lim[:, 1], (n, chain.dof))
    g = rng.uniform(lim[:, 0], lim[:, 1], (n, chain.dof))
    if scale is not None:
        g = s + scale * (g - s)
    return s, g


PLATE = dict(half_extents=(0.0015, 0.35, 0.35), position=(0.45, 0.0, 0.45))


def thin_plate_scene():
    """The Kinova arm and one plate 3 mm thick (a Cuboid), the obstacle discrete checks step over."""
    from numbotics_amd.physics import Cuboid
    from numbotics_amd.scenes import build_scene
    arm, chain, obs = build_scene("c1")
    obs = list(obs) + [Cuboid(0.0, np.array(PLATE["half_extents"]), position=np.array(PLATE["position"]))]
    return arm, chain, obs


def dense_min_distance(orc, s, g, T_f=1.0, n=2000):
    """min over n + 1 samples t in [0, T_f] and over the pairs of the signed distance on the edge s -> g."""
    t = np.linspace(0.0, T_f, n + 1)
    q = (1.0 - t)[:, None] * s[None] + t[:, None] * g[None]
    return pair_distances(orc, q).min()
