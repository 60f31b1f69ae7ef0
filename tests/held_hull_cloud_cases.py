"""Inputs and references of the held-hull-against-point-cloud tests (tests/test_held_hull_cloud_host.py on the CPU,
tests/test_gpu_held_hull_cloud.py on the GPU): a mesh in the hand, held as convex hulls, that sees scans
(``Attachment(..., meshes=True, mesh_scans=True)``, ``engine.DeviceHeld(..., scans=True)``).

The reference is the CPU oracle as it is, on ``held_hull_cases.held_model_hulls(sm, spec, G, world=False, robot=False)`` -- the
scene's model with the held shapes as robot shapes S .. S+H-1 of the holding frame, no pairs, and the held hulls appended to its hull
tables -- through what the primitive held-versus-cloud tests use: ``cloud_cases.cloud_mask`` / ``cloud_closest`` / ``cloud_model``,
``cloud_spline_ref.reference_cloud_splines``, ``cloud_records_cases.Raw`` / ``cut`` and the certified references, each selected on
exactly the held shapes.  A reference is computed once per key and shared.  No test functions here.

The grasps, the H = 8 body and the deep threshold below were picked with the oracle alone; tests/test_held_hull_cloud_host.py pins
what they were picked for."""
import types

import numpy as np

import cloud_cases as cc
import held_cases as hc
import held_cloud_cases as hcc
import held_hull_cases as hh

FIXTURES = ("rock", "tetra", "flat", "mixed", "eight")
SH_HULL = hh.SH_HULL
RESOLUTION = hcc.RESOLUTION
MAXD = hcc.MAXD
BATCHES = hcc.BATCHES                    # (1, 63, 64, 65, 1000)
EDGE_COUNTS = hcc.EDGE_COUNTS            # (1, 63, 64, 65, 200)
SPLINE_COUNTS = (1, 64, 65)
N_ROWS, N_EDGES, N_SPLINES, N_CTRL = 1000, 200, 65, 6
# tc = (thr + 0.001) + r of a held hull (Bullet's 0.001 margin) against the dense scan (r = 0.01): 0.011, 0.021, 0.009 and -0.009 --
# the last is the threshold at which cores_collide_pre's hull_box_far would call every point free and cloud_collides
# goes straight to gjk_collides
THRESHOLDS = (0.0, 0.01, -0.002)
DEEP = -0.02
D_MAX = 0.10
LOOK_AHEADS = (np.inf, 0.05)
MAX_ITER = 64
SPREAD = 0.12                            # of the sampled trajectories' control points about the first (held_traj_cases.SPREAD)
CA_EDGE_SCALE, CA_EDGE_SEED = 0.1, 7     # the certified edges: held_cloud_ca_cases.edges
CA_SPREAD, CA_FIRST = 0.02, 100          # the certified trajectories: held_cloud_ca_cases.splines


def eight_bodies():
    """The H = 8 body: hull, box, hull, sphere, capsule, hull, cylinder, box -- the rock and the wedge among primitives, scattered
    about the first as ``held_cloud_cases.eight_parts`` scatters its parts -> (bodies, grasp)."""
    from numbotics_amd.physics import Mesh, Sphere, Capsule, Cylinder, Cuboid
    rng = np.random.default_rng(8)
    make = (lambda: Mesh(0.0, hh.mesh_path("rock.obj")), lambda: Cuboid(0.0, np.array([0.03, 0.04, 0.05])),
            lambda: Mesh(0.0, hh.mesh_path("wedge.stl")), lambda: Sphere(0.0, 0.05), lambda: Capsule(0.0, 0.03, 0.1),
            lambda: Mesh(0.0, hh.mesh_path("rock.obj")), lambda: Cylinder(0.0, 0.04, 0.1), lambda: Cuboid(0.0, np.array([0.05, 0.03, 0.04])))
    parts = []
    for f in make:
        body = f()
        T = hc.rot_pose(rng, 1.0, 0.0)
        T[:3, 3] = hc.PARK + rng.uniform(-0.25, 0.25, 3)
        body.pose = T
        parts.append(body)
    return parts, hc.trans(0.0, 0.0, 0.3)


def fixture(arm, kind, scans=True):
    """``held_hull_cases.fixture`` with the attachments opted in (``mesh_scans=scans``) and the H = 8 fixture -> (spec, attachment or
    None, what must stay alive)."""
    from numbotics_amd.physics import Mesh, Cuboid
    kw = dict(meshes=True, mesh_scans=True) if scans else dict(meshes=True)
    if kind == "rock":
        body = Mesh(0.0, hh.mesh_path("rock.obj"), position=hc.PARK.copy())
        att = arm.attach(body, "gripper", pose=hh.GRASP[kind], **kw)
        return att.spec(arm), att, body
    if kind == "mixed":
        bodies = [Mesh(0.0, hh.mesh_path("rock.obj"), position=hc.PARK.copy()),
                  Cuboid(0.0, np.array([0.05, 0.05, 0.1]), collision_margin=0.01, position=hc.PARK + np.array([0.0, 0.0, 0.2])),
                  Mesh(0.0, hh.mesh_path("wedge.stl"), position=hc.PARK + np.array([0.0, 0.15, 0.0]))]
        att = arm.attach(bodies, "gripper", pose=hh.GRASP[kind], **kw)
        return att.spec(arm), att, bodies
    if kind == "eight":
        bodies, pose = eight_bodies()
        att = arm.attach(bodies, "gripper", pose=pose, **kw)
        return att.spec(arm), att, bodies
    return hh.fixture(arm, kind)


def scene(name, kind, scans=True):
    """-> namespace(arm, chain, keep, sm, att, spec, q (2000, dof), shapes, base, name, kind) of scene ``name`` (c5m: with the plane
    ``held_hull_cases.scene`` gives it) and fixture ``kind`` in the gripper; ``shapes``: the robot shapes off the base link."""
    from numbotics_amd.physics import Plane
    from numbotics_amd.scenes import build_scene, sample_q
    arm, chain, obs = build_scene(name)
    if name == "c5m":
        obs = list(obs) + [Plane(0.0, np.array([0.0, 0.0, 1.0]), position=np.array([0.0, 0.0, 0.05]))]
        arm.remove_collision_pair("base_link", obs[-1].name)
    spec, att, keep = fixture(arm, kind, scans)
    sm = arm.scene_model()
    base = sm.links[sm.rshape_link[0]]._name
    shapes = [k for k in range(sm.n_rshapes) if sm.links[sm.rshape_link[k]]._name != base]
    return types.SimpleNamespace(arm=arm, chain=chain, keep=(obs, keep), sm=sm, att=att, spec=spec, q=sample_q(chain, 2000, seed=3),
                                 shapes=shapes, base=base, name=name, kind=kind)


def device_held(dev, spec, scans=True):
    from numbotics_amd.engine import DeviceHeld
    return DeviceHeld(dev, spec.frame, spec.A, spec.G, spec.shape_type, spec.shape_local, spec.shape_param, spec.world_shapes,
                      spec.robot_shapes, hulls=spec.hulls, scans=scans)


def device(x, scans=True):
    """-> (DeviceModel, DeviceHeld) of ``x``: the attachment's own where there is one, else made from the spec."""
    if x.att is not None and scans:
        return x.att._device(x.arm)
    _, dev = x.arm._scene_device()
    return dev, device_held(dev, x.spec, scans)


# ---- the parity model and the references on it
def robot_model(sm, spec, G=None):
    """-> (the combined descriptor with no pairs, the held shapes' indices S .. S+H-1)."""
    hm = hh.held_model_hulls(sm, spec, G, world=False, robot=False)
    return hm, list(range(sm.n_rshapes, sm.n_rshapes + spec.n_shapes))


def one_shape(spec, h):
    """``spec`` cut to held shape h (the hull tables stay whole: the hull index still names its hull)."""
    import dataclasses
    return dataclasses.replace(spec, shape_local=spec.shape_local[h:h + 1], shape_type=spec.shape_type[h:h + 1],
                               shape_param=np.asarray(spec.shape_param).reshape(-1, 4)[h:h + 1])


def mask(sm, spec, pts, r, q, thr, G=None):
    hm, shapes = robot_model(sm, spec, G)
    return cc.cloud_mask(hm, pts, r, q, thr, shapes=shapes)


def mask_rows(sm, spec, pts, r, q, thr, G):
    return np.array([mask(sm, spec, pts, r, q[b], thr, G[b])[0] for b in range(q.shape[0])], dtype=bool)


def closest(sm, spec, pts, r, q, d_max, G=None):
    hm, shapes = robot_model(sm, spec, G)
    d, s, p = cc.cloud_closest(hm, pts, r, q, d_max, shapes=shapes)
    return d, np.where(s >= 0, s - sm.n_rshapes, -1).astype(np.int32), p


def edges_ref(sm, spec, pts, r, s, g, maxd=MAXD, mode="connect", thr=0.0, dist=None, G=None):
    from oracle.cpu_oracle import Oracle
    hm, shapes = robot_model(sm, spec, G)
    return Oracle(cc.cloud_model(hm, pts, r, shapes)).edge_validity(s, g, RESOLUTION, maxd, mode=mode, threshold=thr, dist=dist, nthreads=8)


def splines_ref(sm, spec, pts, r, ctrl, knots, k, thr=0.0, G=None, status=0, prev=None):
    from cloud_spline_ref import reference_cloud_splines
    hm, shapes = robot_model(sm, spec, G)
    return reference_cloud_splines(hm, pts, r, ctrl, knots, k, RESOLUTION, thr, shapes=shapes, status=status, prev=prev)


def records_raw(x, pts, r, q, G=None):
    import cloud_records_cases as crc
    hm, shapes = robot_model(x.sm, x.spec, G)
    return crc.Raw(hm, pts, r, q, shapes)


def records_ref(x, raw, d_max, per_shape):
    import cloud_records_cases as crc
    d, s, p, w, j = crc.cut(raw, d_max, per_shape)
    return d, np.where(s >= 0, s - x.sm.n_rshapes, -1).astype(np.int32), p, w, j


def edge_ca_ref(x, pts, r, s, g, maxd=MAXD, mode="connect", thr=0.0, look_ahead=np.inf, dist=None, G=None):
    """valid, end, t_free, status, item stops, item statuses, exits of the held-versus-cloud items alone."""
    from cloud_continuous_ref import reference_cloud_continuous
    hm, shapes = robot_model(x.sm, x.spec, G)
    return reference_cloud_continuous(hm, pts, r, s, g, maxd, mode=mode, threshold=thr, max_iter=MAX_ITER, slack=1e-6,
                                      look_ahead=look_ahead, dist=dist, shapes=shapes)


def spline_ca_ref(x, pts, r, ctrl, knots, k, thr=0.0, look_ahead=np.inf, G=None):
    """valid, t_free, status, item stops, item statuses, exits of the held-versus-cloud items alone."""
    from cloud_spline_continuous_ref import reference_cloud_spline_continuous
    hm, shapes = robot_model(x.sm, x.spec, G)
    return reference_cloud_spline_continuous(hm, pts, r, ctrl, knots, k, threshold=thr, max_iter=MAX_ITER, slack=1e-6,
                                             look_ahead=look_ahead, shapes=shapes)


# ---- inputs
def edges(x, E=N_EDGES):
    """E edges a -> a + U(-0.5, 0.5) (``held_cases.edge_set``)."""
    return hc.edge_set(x.q, E)


def splines(x, degree, S=N_SPLINES, n=N_CTRL):
    """S sampled trajectories: the first control point a sampled configuration, the others scattered about it."""
    from numbotics_amd.planning import unit_knots
    rng = np.random.default_rng(17)
    ctrl = x.q[:S, None, :] + rng.uniform(-SPREAD, SPREAD, (S, n, x.chain.dof))
    ctrl[:, 0, :] = x.q[:S]
    return np.ascontiguousarray(ctrl), unit_knots(n, degree)


def ca_edges(x, E=N_EDGES):
    """The certified tests' short edges a -> a + U(-0.1, 0.1) (``held_cloud_ca_cases.edges``)."""
    rng = np.random.default_rng(CA_EDGE_SEED)
    s = x.q[:E].copy()
    return s, s + rng.uniform(-CA_EDGE_SCALE, CA_EDGE_SCALE, s.shape)


def ca_splines(x, degree, S=N_SPLINES, n=8):
    """The certified tests' trajectories: a random walk from a sampled configuration (``held_cloud_ca_cases.splines``)."""
    from numbotics_amd.planning import unit_knots
    step = np.random.default_rng(7).uniform(-CA_SPREAD, CA_SPREAD, (S, n, x.chain.dof))
    return x.q[CA_FIRST:CA_FIRST + S, None, :] + np.cumsum(step, axis=1), unit_knots(n, degree)


def deep_points(x, pts, rows, G=None, link="gripper"):
    """``pts`` with one point added at the local origin of the first held hull (the mean of its vertices: inside it) at each of
    ``rows`` (rows of x.q): points deep inside a hull, so that the verdicts at a threshold with tc <= 0 are mixed whatever the
    scan."""
    from oracle.cpu_oracle import Oracle
    h = int(np.flatnonzero(np.asarray(x.spec.shape_type) == SH_HULL)[0])
    T = Oracle(x.sm).fk(x.q[list(rows)], link, extra_local=(x.spec.G if G is None else G) @ x.spec.shape_local[h])
    return np.ascontiguousarray(np.concatenate((np.asarray(pts, dtype=np.float64).reshape(-1, 3), T[:, :3, 3])))


# ---- the case the feature exists for: a held rock carried through a scanned wall, the arm and the scene clear
def wall_edge(x, n_try=400, seed=11):
    """``held_cloud_ca_cases.wall_edge`` on the combined descriptor of ``x`` (a held mesh) -> (wall points, radius, start, goal, the
    held shapes' t_free, the crossing), or None: an edge that the scene, the arm against the wall and the held object against the
    scene all certify FREE while the held object against the wall has status COLLISION.  Chosen with the references alone."""
    from oracle.cpu_oracle import Oracle
    from cloud_continuous_ref import plate_wall, reference_cloud_continuous
    from continuous_ref import reference_continuous, pair_distances
    from ca_ref import FREE, COLLISION
    import held_cloud_ca_cases as hca
    pts = np.ascontiguousarray(plate_wall(hca.WALL_SPACING))
    r = hca.WALL_RADIUS
    rng = np.random.default_rng(seed)
    s = x.q[:n_try].copy()
    g = s + rng.uniform(-0.5, 0.5, s.shape)
    kw = dict(mode="connect", threshold=0.0, max_iter=MAX_ITER, slack=1e-6)
    held = edge_ca_ref(x, pts, r, s, g)
    cand = np.flatnonzero(held[3] == COLLISION)
    if cand.size == 0:
        return None
    s, g, tf = s[cand], g[cand], held[2][cand]
    arm = reference_cloud_continuous(x.sm, pts, r, s, g, MAXD, shapes=x.shapes, **kw)
    both = hh.held_model_hulls(x.sm, x.spec, keep_scene=True)
    scene_ = reference_continuous(both, Oracle(both), s, g, MAXD, **kw)
    hm, shapes = robot_model(x.sm, x.spec)
    orc = Oracle(cc.cloud_model(hm, pts, r, shapes))
    t = np.linspace(0.0, 1.0, 201)
    for e in np.flatnonzero((arm[3] == FREE) & (scene_[3] == FREE)):
        d = pair_distances(orc, (1.0 - t)[:, None] * s[e][None] + t[:, None] * g[e][None]).min(axis=1)
        cross = float(t[int(np.argmin(d))])
        if cross > 0.05 and d.min() < 0.0:
            return pts, r, s[e].copy(), g[e].copy(), float(tf[e]), cross
    return None
