"""Inputs and references of the certified held-object-against-point-cloud tests (tests/test_held_cloud_ca_host.py on the CPU,
tests/test_gpu_held_cloud_ca.py on the GPU).

The references are the NumPy + CPU-oracle restatements of the cloud's certified entries as they are
(cloud_continuous_ref.reference_cloud_continuous, cloud_spline_continuous_ref.reference_cloud_spline_continuous), on
``held_cloud_cases.held_robot_model``: the scene's model with the held shapes as robot shapes S .. S+H-1 of the holding frame and no
pairs, selected on exactly those shapes.  They are the slow part, so each is computed once per argument set and shared
(``held_cloud_cases.shared``); per-trajectory results do not depend on the batch, so a prefix of a set is a prefix of its reference.
No test functions here."""
import types

import numpy as np

import held_cases as hc
import held_cloud_cases as hcc
import held_traj_cases as ht

MAXD = hcc.MAXD                      # connect: no edge is cut short
MAXD_STEER = 0.12                    # steer: about half of the edges are cut at T_f < 1
EDGE_SCALE, EDGE_SEED = 0.1, 7       # edges a -> a + U(-0.1, 0.1): a mid-edge contact stops UNDECIDED (the advance converges on it from the
                                     # free side), so short edges keep that share low; picked with the reference (worst of the 16 sets of
                                     # 200: 151 FREE, 23 COLLISION, 5 UNDECIDED)
EDGE_COUNTS = hcc.EDGE_COUNTS        # (1, 63, 64, 65, 200)
N_EDGES = hcc.N_EDGES
SPLINE_COUNTS = (1, 64, 65, 100)
N_SPLINES, N_CTRL = 100, 8
THRESHOLDS = (0.0, 0.01)
LOOK_AHEADS = (np.inf, 0.05)         # (the default is inf)
MAX_ITER = 64
# the first sampled configuration the splines start from and the spread of the control points' random walk: picked with the reference
# so that every set of 100 has at least 10 % FREE, at least 10 % COLLISION and at most 5 % UNDECIDED (worst of the 20 sets: 73 / 15 /
# 4; tests/test_held_cloud_ca_host.py pins the conditions without a GPU)
SPLINE_FIRST, SPREAD = 100, 0.02


def scene(name, att=None):
    """-> namespace(arm, chain, keep, sm, att, spec, q (2000, dof), shapes, base): ``name`` with the parity fixtures' box on the
    gripper (``att(arm)`` -> (attachment, keep-alive) puts something else there); ``shapes``: the robot shapes off the base link, which
    stands on the scanned table."""
    from numbotics_amd.scenes import build_scene, sample_q
    arm, chain, obs = build_scene(name)
    a, b = hc.gripper_box(arm) if att is None else att(arm)
    sm = arm.scene_model()
    base = sm.links[sm.rshape_link[0]]._name
    shapes = [k for k in range(sm.n_rshapes) if sm.links[sm.rshape_link[k]]._name != base]
    return types.SimpleNamespace(arm=arm, chain=chain, keep=(obs, b), sm=sm, att=a, spec=a.spec(arm), q=sample_q(chain, 2000, seed=3),
                                 shapes=shapes, base=base)


def kind_att(kind):
    def make(arm):
        body = hcc.kind_bodies()[kind]
        return arm.attach(body, "gripper", pose=hc.trans(0.0, 0.0, hc.BOX_Z)), body
    return make


def eight_att(arm):
    parts, pose = hcc.eight_parts()
    return arm.attach(parts, "gripper", pose=pose), parts


def edges(x, E=N_EDGES):
    """E edges a -> a + U(-EDGE_SCALE, EDGE_SCALE) from the scene's sampled configurations."""
    rng = np.random.default_rng(EDGE_SEED)
    s = x.q[:E].copy()
    return s, s + rng.uniform(-EDGE_SCALE, EDGE_SCALE, s.shape)


def special_edges(x, E=N_EDGES):
    """``edges`` with a degenerate edge (7)."""
    s, g = edges(x, E)
    g[7] = s[7]
    return s, g


def nan_edges(x, E=N_EDGES):
    """-> starts, goals, dist: ``special_edges`` with a NaN in a start row (11) and the lengths given (1.1 times the norm: the norm
    of a row that is not finite is not a length, and the edge would be degenerate)."""
    s, g = special_edges(x, E)
    dist = 1.1 * np.linalg.norm(g - s, axis=1)
    s[11, 3] = np.nan
    return s, g, dist


def splines(x, degree=3, S=N_SPLINES, n=N_CTRL):
    """-> ctrl (S, n, dof), knots: the first control point a sampled configuration, the others a random walk from it."""
    from numbotics_amd.planning import unit_knots
    step = np.random.default_rng(7).uniform(-SPREAD, SPREAD, (S, n, x.chain.dof))
    return x.q[SPLINE_FIRST:SPLINE_FIRST + S, None, :] + np.cumsum(step, axis=1), unit_knots(n, degree)


def edge_reference(x, pts, r, s, g, maxd, mode="connect", thr=0.0, look_ahead=np.inf, dist=None, G=None, scene_orc=None,
                   max_iter=MAX_ITER):
    """valid, end, t_free, status, item stops, item statuses, exits of the held-versus-cloud items alone (``scene_orc``: see
    ``four_step_edges``)."""
    from cloud_continuous_ref import reference_cloud_continuous
    hm, shapes = hcc.held_robot_model(x.sm, x.spec, G)
    return reference_cloud_continuous(hm, pts, r, s, g, maxd, mode=mode, threshold=thr, max_iter=max_iter, slack=1e-6,
                                      look_ahead=look_ahead, dist=dist, shapes=shapes, scene_orc=scene_orc)


@hcc.shared
def _edge_ref(x, name, scan, mode, thr, look_ahead, special):
    pts, r = hcc.scan(scan)
    s, g = special_edges(x) if special else edges(x)
    return edge_reference(x, pts, r, s, g, MAXD if mode == "connect" else MAXD_STEER, mode, thr, look_ahead)


def edge_ref(x, name, scan, mode="connect", thr=0.0, look_ahead=np.inf, special=False):
    """The reference of the N_EDGES edges of fixture ``name`` (``scene(name)`` with the gripper box; another body: give it a name of
    its own) against scan ``scan``: computed once per argument set."""
    return _edge_ref(x, name, scan, mode, float(thr), float(look_ahead), bool(special))


def spline_reference(x, pts, r, ctrl, knots, k, thr=0.0, look_ahead=np.inf, G=None, scene_orc=None, per_span_cut=False,
                     max_iter=MAX_ITER):
    """valid, t_free, status, item stops, item statuses, exits of the held-versus-cloud items alone."""
    from cloud_spline_continuous_ref import reference_cloud_spline_continuous
    hm, shapes = hcc.held_robot_model(x.sm, x.spec, G)
    return reference_cloud_spline_continuous(hm, pts, r, ctrl, knots, k, threshold=thr, max_iter=max_iter, slack=1e-6,
                                             look_ahead=look_ahead, shapes=shapes, scene_orc=scene_orc, per_span_cut=per_span_cut)


@hcc.shared
def _spline_ref(x, name, scan, degree, thr, look_ahead):
    pts, r = hcc.scan(scan)
    ctrl, knots = splines(x, degree)
    return spline_reference(x, pts, r, ctrl, knots, degree, thr, look_ahead)


def spline_ref(x, name, scan, degree=3, thr=0.0, look_ahead=np.inf):
    return _spline_ref(x, name, scan, int(degree), float(thr), float(look_ahead))


def four_step_items(x, pts, r, s, g, maxd, mode="connect", thr=0.0, look_ahead=np.inf, dist=None, G=None, max_iter=MAX_ITER):
    """The item stop points and statuses of the four certified steps on the edges s -> g, each (E, items): the scene's pairs, the
    arm's shapes (``x.shapes``) against the scan, the held items against the scene, the held shapes against the scan -> (stops,
    statuses, Tf, live), lists of four."""
    from oracle.cpu_oracle import Oracle
    from cloud_continuous_ref import reference_cloud_continuous
    from continuous_ref import reference_continuous, edge_span
    kw = dict(mode=mode, threshold=thr, max_iter=max_iter, slack=1e-6, dist=dist)
    a = reference_continuous(x.sm, Oracle(x.sm), s, g, maxd, **kw)
    b = reference_cloud_continuous(x.sm, pts, r, s, g, maxd, look_ahead=look_ahead, shapes=x.shapes, **kw)
    hm = hc.held_model(x.sm, x.spec, G)
    c = reference_continuous(hm, Oracle(hm), s, g, maxd, **kw)
    d = edge_reference(x, pts, r, s, g, maxd, mode, thr, look_ahead, dist, G, max_iter=max_iter)
    spans = [edge_span(s[e], g[e], None if dist is None else dist[e], maxd, mode) for e in range(s.shape[0])]
    live = np.array([sp is not None for sp in spans], dtype=bool)
    Tf = np.array([sp[1] if sp is not None else np.nan for sp in spans])
    return [a[4], b[4], c[4], d[4]], [a[5], b[5], c[5], d[5]], Tf, live


def reduce_steps(stops, statuses, Tf, live, n):
    """valid, t_free, status of one certified call over the items of the first ``n`` steps together."""
    from ca_ref import reduce_items
    return reduce_items(np.concatenate(stops[:n], axis=1), np.concatenate(statuses[:n], axis=1), Tf, live)


def four_step_spline_items(x, pts, r, ctrl, knots, k, thr=0.0, look_ahead=np.inf, G=None):
    """``four_step_items`` for trajectories -> (stops, statuses, live)."""
    from oracle.cpu_oracle import Oracle
    from cloud_spline_continuous_ref import reference_cloud_spline_continuous
    from spline_continuous_ref import reference_spline_continuous, degenerate
    kw = dict(threshold=thr, max_iter=MAX_ITER, slack=1e-6)
    a = reference_spline_continuous(x.sm, Oracle(x.sm), ctrl, knots, k, **kw)
    b = reference_cloud_spline_continuous(x.sm, pts, r, ctrl, knots, k, look_ahead=look_ahead, shapes=x.shapes, **kw)
    hm = hc.held_model(x.sm, x.spec, G)
    c = reference_spline_continuous(hm, Oracle(hm), ctrl, knots, k, **kw)
    d = spline_reference(x, pts, r, ctrl, knots, k, thr, look_ahead, G)
    return [a[3], b[3], c[3], d[3]], [a[4], b[4], c[4], d[4]], ~degenerate(ctrl, np.asarray(knots, dtype=np.float64), k)


def shares(status):
    """(FREE, COLLISION, UNDECIDED) counts of a certified status array."""
    return ht.shares(status)


def assert_shares(status, what):
    """The conditions every set of 100 or more trajectories meets on the REFERENCE: at least 10 % FREE, at least 10 % COLLISION, at
    most 5 % UNDECIDED."""
    n = len(status)
    f, c, u = shares(status)
    assert n >= 100 and 10 * f >= n and 10 * c >= n and 20 * u <= n, f"{what}: {f} FREE / {c} COLLISION / {u} UNDECIDED of {n}"


# ---- the mu_max case: a slow first span and a fast later one that reaches a point
def fast_last_span(x, r=0.01):
    """One trajectory of 6 control points, degree 3 (three spans): the first four control points creep (1e-4 per leg), the last two
    swing the shoulder by 1.2 -- the last span is the fast one -- into ONE point, placed inside the held box at q(1) and more than
    0.1 from it up to t = 0.795 -> (trajectory (1, 6, n_q), knots, 3, the point (1, 3), its radius)."""
    from numbotics_amd.planning import unit_knots
    from oracle.cpu_oracle import Oracle
    from cloud_cases import cloud_model
    from continuous_ref import pair_distances
    from spline_ref import de_boor
    kn, k = unit_knots(6, 3), 3
    hm, shapes = hcc.held_robot_model(x.sm, x.spec)
    box = np.random.default_rng(8).uniform([-1.2, -1.2, -0.2], [1.2, 1.2, 1.6], (100000, 3))
    t = np.linspace(0.0, 1.0, 201)
    for q0 in x.q[:16]:
        c = np.repeat(q0[None], 6, axis=0)
        c[1:4, 1] += 1e-4 * np.arange(1, 4)
        c[4, 1] += 0.6
        c[5, 1] += 1.2
        q = de_boor(c[None], kn, k, np.zeros(t.shape[0], dtype=np.int64), t)
        cand = box[pair_distances(Oracle(cloud_model(hm, box, r, shapes)), q[-1:])[0] < -0.002]      # inside the box at q(1)
        if cand.shape[0] == 0:
            continue
        d = pair_distances(Oracle(cloud_model(hm, cand, r, shapes)), q)                              # (201, candidates)
        ok = d[:160].min(axis=0) > 0.1
        if ok.any():
            return c[None], kn, k, cand[np.nonzero(ok)[0][:1]], r
    raise AssertionError("no point is hit at the end only")


# ---- the case this feature exists for: a held box carried through a scanned wall, the arm and the scene clear
WALL_SPACING = 0.05
WALL_RADIUS = 0.01


def wall_edge(x, n_try=400, seed=11):
    """-> (wall points, radius, start, goal, the held items' t_free, the crossing): an edge of scene ``x`` (the gripper box) that the
    scene, the arm against the wall and the held box against the scene all certify FREE while the held box against the wall has
    status COLLISION -- the box reaches into the wall's shell where the edge starts (the advance converges on a contact further along
    from its free side and stops UNDECIDED there) -- and goes on through it: the crossing, where the box is deepest in the wall, lies
    further along than 0.05.  Chosen with the references alone."""
    from oracle.cpu_oracle import Oracle
    from cloud_cases import cloud_model
    from cloud_continuous_ref import plate_wall, reference_cloud_continuous
    from continuous_ref import reference_continuous, pair_distances
    from ca_ref import FREE, COLLISION
    pts = np.ascontiguousarray(plate_wall(WALL_SPACING))
    rng = np.random.default_rng(seed)
    s = x.q[:n_try].copy()
    g = s + rng.uniform(-0.5, 0.5, s.shape)
    kw = dict(mode="connect", threshold=0.0, max_iter=MAX_ITER, slack=1e-6)
    held = edge_reference(x, pts, WALL_RADIUS, s, g, MAXD)
    cand = np.flatnonzero(held[3] == COLLISION)
    if cand.size == 0:
        return None
    s, g, tf = s[cand], g[cand], held[2][cand]
    arm = reference_cloud_continuous(x.sm, pts, WALL_RADIUS, s, g, MAXD, shapes=x.shapes, **kw)
    both = hc.held_model(x.sm, x.spec, keep_scene=True)
    scene_ = reference_continuous(both, Oracle(both), s, g, MAXD, **kw)
    hm, shapes = hcc.held_robot_model(x.sm, x.spec)
    orc = Oracle(cloud_model(hm, pts, WALL_RADIUS, shapes))
    t = np.linspace(0.0, 1.0, 201)
    for e in np.flatnonzero((arm[3] == FREE) & (scene_[3] == FREE)):
        d = pair_distances(orc, (1.0 - t)[:, None] * s[e][None] + t[:, None] * g[e][None]).min(axis=1)
        cross = float(t[int(np.argmin(d))])
        if cross > 0.05 and d.min() < 0.0:
            return pts, WALL_RADIUS, s[e].copy(), g[e].copy(), float(tf[e]), cross
    return None
