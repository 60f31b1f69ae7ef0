"""Held objects, the part that needs no device: the host twin of the kernels' local-pose products against its NumPy restatement,
``Arm.attach``'s pair resolution, default pose and errors, ``World.add_constraint``, the refusals of ``ConnectorParams(attached=...)``,
the header / binding agreement, and the conditions of the GPU tests' fixtures (tests/held_cases.py) by the CPU oracle."""
import os
import re

import numpy as np
import pytest

from numbotics_amd import _lib
from numbotics_amd.scenes import build_scene, sample_q
import held_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nbk_held_locals_host", "nbk_held_create", "nbk_held_destroy", "nbk_held_validity_batch", "nbk_edge_held_workspace_bytes",
           "nbk_edge_held_validity_batch")


def test_symbols_declared_and_bound():
    with open(os.path.join(ROOT, "include", "nbk.h")) as f:
        declared = set(re.findall(r"\b(nbk_\w+)\s*\(", f.read()))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
    assert lib.nbk_edge_held_workspace_bytes(-1) < 0
    for E in (0, 1, 300):                                       # the 40-byte-per-edge plan of the cloud's sampled edges
        assert lib.nbk_edge_held_workspace_bytes(E) == lib.nbk_edge_cloud_workspace_bytes(E) >= 40 * E


def test_build_tracks_the_header():
    from numbotics_amd.csrc import build
    import inspect
    assert "nbk_held.hpp" in build.SOURCES and '"nbk_held.hpp"' in inspect.getsource(build.source_digest)


def test_locals_host_is_the_restatement_bit_for_bit():
    from numbotics_amd.engine import held_locals
    rng = np.random.default_rng(17)
    for trial in range(20):
        A, G = hc.rot_pose(rng, 3.0, 1.0), hc.rot_pose(rng, 3.0, 1.0)
        L = np.array([hc.rot_pose(rng, 3.0, 1.0) for _ in range(1 + trial % 8)])
        got, ref = held_locals(A, G, L), hc.locals_ref(A, G, L)
        assert got.shape == ref.shape == (L.shape[0], 3, 4)
        assert np.array_equal(got.view(np.int64), ref.view(np.int64)), trial
        # the fused products differ from NumPy's separately rounded ones somewhere: the restatement is not vacuous
    plain = np.array([((A @ G) @ Lh)[:3] for Lh in L])
    assert not np.array_equal(plain.view(np.int64), ref.view(np.int64))
    assert np.allclose(plain, ref, rtol=0, atol=1e-14)
    # argument rules
    lib = _lib.load()
    a = np.zeros(12)
    assert lib.nbk_held_locals_host(None, a.ctypes.data, a.ctypes.data, 1, a.ctypes.data) == -1
    assert lib.nbk_held_locals_host(a.ctypes.data, a.ctypes.data, None, 1, a.ctypes.data) == -1
    assert lib.nbk_held_locals_host(a.ctypes.data, a.ctypes.data, None, 0, None) == 0
    assert lib.nbk_held_locals_host(a.ctypes.data, a.ctypes.data, a.ctypes.data, -1, a.ctypes.data) == -1


def test_create_argument_rules_need_no_device():
    import ctypes as C
    lib = _lib.load()
    out = C.c_void_p(123)
    a = np.zeros(12)
    assert lib.nbk_held_create(None, 0, a.ctypes.data, a.ctypes.data, 1, a.ctypes.data, a.ctypes.data, a.ctypes.data, 0, None, None,
                               C.byref(out)) == -1
    assert out.value is None
    lib.nbk_held_destroy(None)
    assert lib.nbk_held_validity_batch(None, None, None, 0, None, 0, 0.0, 0, None, None, None) == -1
    assert lib.nbk_edge_held_validity_batch(None, None, None, None, None, 0, 0.05, 1.0, 0, 0.0, None, 0, None, None, None, None, 0, None) == -1


def test_attach_pair_resolution(fresh_world):
    arm, chain, obs = build_scene("c3")
    att, b = hc.gripper_box(arm)
    sm, spec = arm.scene_model(), att.spec(arm)
    link_of = lambda s: sm.links[sm.rshape_link[s]]._name      # noqa: E731
    assert sm.n_wshapes == 9 and sm.objects[sm.wshape_obj[8]] is b
    assert list(spec.world_shapes) == list(range(8)), "the object's own world shape is excluded"
    fr = sm.kin.frames["gripper"]
    assert spec.frame == fr.joint == 6 and np.array_equal(spec.A, fr.local) and np.array_equal(spec.G, hc.trans(0, 0, hc.BOX_Z))
    # the holding link and everything on its moving frame (bracelet, the gripper base) are exempt
    assert [link_of(s) for s in spec.robot_shapes] == ["base_link", "shoulder_link", "half_arm_1_link", "half_arm_2_link", "forearm_link",
                                                      "spherical_wrist_1_link", "spherical_wrist_2_link"]
    assert all(sm.rshape_frame[s] != 6 for s in spec.robot_shapes)
    att2 = arm.attach(b, chain._links[[l._name for l in chain._links].index("gripper")], pose=np.eye(4),
                      touch_links=("spherical_wrist_2_link", arm._resolve("forearm_link")))
    assert [link_of(s) for s in att2.spec(arm).robot_shapes] == ["base_link", "shoulder_link", "half_arm_1_link", "half_arm_2_link",
                                                                "spherical_wrist_1_link"]
    # the shape record: the descriptor's shape mode, an explicit margin wins
    assert spec.n_shapes == 1 and spec.shape_type[0] == hc.SH_BOX and np.array_equal(spec.shape_param[0], [0.1, 0.1, 0.2, 0.04])
    plain = arm.attach(_cuboid((0.1, 0.1, 0.2)), "gripper", pose=np.eye(4))
    assert plain.spec(arm).shape_param[0, 3] == pytest.approx(0.01), "Bullet's margin: a tenth of the smallest half extent"
    arm.bullet_margins = False
    assert plain.spec(arm).shape_param[0, 3] == 0.0, "re-resolved with the scene: sharp"
    # the cache: one spec per scene state
    s1 = att.spec(arm)
    assert att.spec(arm) is s1
    obs[0].position = np.array([2.0, 0.0, 0.0])
    assert att.spec(arm) is not s1


def _cuboid(half, **kw):
    from numbotics_amd.physics import Cuboid
    return Cuboid(0.0, np.array(half, dtype=np.float64), position=hc.PARK.copy(), **kw)


def test_attach_default_pose_and_lists(fresh_world):
    from numbotics_amd.physics import Sphere, Capsule, Cylinder
    from numbotics_amd.robots.model import chain_link_poses
    arm, chain, obs = build_scene("c2")
    arm.configuration = sample_q(chain, 1, seed=9)[0]
    b = _cuboid((0.05, 0.06, 0.07))
    T = hc.rot_pose(np.random.default_rng(3), 1.0, 0.5)
    b.pose = T
    att = arm.attach(b, "gripper")
    assert np.allclose(chain_link_poses(chain)["gripper"] @ att.pose, T, rtol=0, atol=1e-12), "the object where it stands now"
    # a list: the first object's frame, the others relative to it
    parts = [b, Sphere(0.0, 0.03), Capsule(0.0, 0.02, 0.1), Cylinder(0.0, 0.03, 0.08)]
    parts[1].pose = T @ hc.trans(0.1, 0.0, 0.0)
    parts[2].pose = T @ hc.trans(0.0, 0.1, 0.0)
    parts[3].pose = T @ hc.trans(0.0, 0.0, 0.1)
    att = arm.attach(parts, "gripper")
    spec = att.spec(arm)
    assert list(spec.shape_type) == [hc.SH_BOX, hc.SH_SPHERE, hc.SH_CAPSULE, hc.SH_CYLINDER]
    assert np.array_equal(spec.shape_local[0], np.eye(4))
    for k, t in ((1, (0.1, 0, 0)), (2, (0, 0.1, 0)), (3, (0, 0, 0.1))):
        assert np.allclose(spec.shape_local[k], hc.trans(*t), rtol=0, atol=1e-12)
    sm = arm.scene_model()
    held = {id(p) for p in parts}
    assert all(id(sm.objects[sm.wshape_obj[w]]) not in held for w in spec.world_shapes) and len(spec.world_shapes) == sm.n_wshapes - 4


def test_attach_errors(fresh_world):
    from numbotics_amd.physics import Plane, Mesh, Sphere
    from numbotics_amd.scenes import MESH_DIR
    arm, chain, obs = build_scene("c2")
    b = _cuboid((0.05, 0.05, 0.05))
    with pytest.raises(ValueError):
        arm.attach(b, "no_such_link")
    with pytest.raises(ValueError):
        arm.attach(b, obs[0])                                   # an object is no link
    with pytest.raises(ValueError, match="not found in chain"):
        arm.attach(b, "gripper", touch_links=("no_such_link",))
    with pytest.raises(ValueError, match="PLANE"):
        arm.attach(Plane(0.0, np.array([0.0, 0.0, 1.0])), "gripper", pose=np.eye(4))
    with pytest.raises(ValueError, match="MESH"):
        arm.attach(Mesh(0.0, os.path.join(MESH_DIR, "rock.obj")), "gripper", pose=np.eye(4))
    with pytest.raises(ValueError, match="at most 8"):
        arm.attach([Sphere(0.0, 0.01) for _ in range(9)], "gripper", pose=np.eye(4))
    with pytest.raises(ValueError):
        arm.attach([], "gripper", pose=np.eye(4))
    with pytest.raises(ValueError):
        arm.attach("not an object", "gripper", pose=np.eye(4))
    with pytest.raises(ValueError, match="finite"):
        arm.attach(b, "gripper", pose=np.full((4, 4), np.nan))
    with pytest.raises(ValueError):
        arm.attach(b, "gripper", pose=np.eye(3))
    assert len(arm.attach([Sphere(0.0, 0.01) for _ in range(8)], "gripper", pose=np.eye(4)).spec(arm).shape_type) == 8


def test_add_constraint(fresh_world):
    from numbotics_amd.physics import Joint, Constraint, Attachment
    arm, chain, obs = build_scene("c2")
    w = chain.world
    link = arm._resolve("gripper")
    b = _cuboid((0.05, 0.05, 0.05))
    rng = np.random.default_rng(5)
    off, P, Cp = hc.rot_pose(rng), hc.rot_pose(rng), hc.rot_pose(rng)
    assert w.attachments() == []
    a1 = w.add_constraint(link, b, Joint(off, np.zeros(3), Constraint.FIXED, parent_pose=P, child_pose=Cp))
    a2 = w.add_constraint(b, link, Joint(off, np.zeros(3), Constraint.FIXED, parent_pose=P, child_pose=Cp))
    a3 = w.add_constraint(link, b, Joint(off, np.zeros(3), Constraint.FIXED))
    assert w.attachments() == [a1, a2, a3] and all(isinstance(a, Attachment) for a in (a1, a2, a3))
    assert a1.link is link and a1.objects == (b,) and a2.link is link and a2.objects == (b,)
    # the two frames the reference hands Bullet coincide: T_link (off P) = T_obj (off C)
    assert np.allclose(a1.pose @ (off @ Cp), off @ P, rtol=0, atol=1e-12)
    assert np.allclose(a2.pose @ (off @ P), off @ Cp, rtol=0, atol=1e-12)
    assert np.allclose(a3.pose, np.eye(4), rtol=0, atol=1e-12)
    assert list(a1.spec(arm).world_shapes) == [0]               # resolved by the arm that owns the link
    for bad in (Constraint.PRISMATIC, Constraint.REVOLUTE, Constraint.SPHERICAL):
        with pytest.raises(NotImplementedError):
            w.add_constraint(link, b, Joint(off, np.array([0.0, 0.0, 1.0]), bad))
    fixed = Joint(off, np.zeros(3), Constraint.FIXED)
    for x, y in ((b, obs[0]), (link, arm._resolve("forearm_link")), (chain, b), (link, chain)):
        with pytest.raises(NotImplementedError):
            w.add_constraint(x, y, fixed)
    assert len(w.attachments()) == 3
    # an attachment on a link of another chain is refused by the arm
    arm_b, chain_b, _ = build_scene("c1")
    with pytest.raises(ValueError, match="not found in chain"):
        a1.spec(arm_b)


def test_connector_params_refusals(fresh_world):
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, DiscreteConnector, ContinuousConnector
    from numbotics_amd.planning import unit_bspline
    arm, chain, obs = build_scene("c2")
    att, b = hc.gripper_box(arm)
    with pytest.raises(ValueError, match="needs ConnectorParams"):
        ConnectorParams(validity_checker=lambda q: True, attached=att)
    p = ConnectorParams(arm=arm, attached=att)
    assert p.attached is att and ConnectorParams(arm=arm).attached is None
    with pytest.raises(ValueError, match="do not see held objects yet"):
        ContinuousConnector(p)
    con = DiscreteConnector(p)
    q = sample_q(chain, 4, seed=1)
    with pytest.raises(ValueError, match="do not see held objects yet"):
        con.validate_trajectories(q[None], degree=1)
    with pytest.raises(ValueError, match="do not see held objects yet"):
        con.validate_trajectory(unit_bspline(q))


@pytest.mark.parametrize("name", ("c3", "c2"))
def test_fixture_conditions_validity(fresh_world, name):
    """In every parity fixture the share of rows the held pairs alone decide as colliding lies in [10 %, 90 %] by the oracle."""
    arm, chain, obs = build_scene(name)
    att, b = hc.gripper_box(arm)
    sm, spec = arm.scene_model(), att.spec(arm)
    q = sample_q(chain, 2000, seed=3)
    for thr in hc.THRESHOLDS:
        share = float(hc.held_mask(sm, spec, q, thr).mean())
        print(f"{name} thr={thr}: held pairs collide in {share:.4f} of 2000 rows")
        assert 0.10 <= share <= 0.90, (name, thr, share)
        for B in hc.BATCHES[1:]:
            assert 0 < hc.held_mask(sm, spec, q[:B], thr).sum() < B, (name, thr, B)


def test_fixture_conditions_edges(fresh_world):
    arm, chain, obs = build_scene("c3")
    att, b = hc.gripper_box(arm)
    sm, spec = arm.scene_model(), att.spec(arm)
    s, g = hc.edge_set(sample_q(chain, 2000, seed=3), 300)
    valid, end, ns = hc.held_edges_ref(sm, spec, s, g, 0.05, 10.0)
    print(f"c3 edges: {valid.mean():.4f} valid, at most {ns.max()} samples")
    assert 0.10 <= float(valid.mean()) <= 0.90 and ns.max() <= 23
    assert 0 < valid[:65].sum() < 65


def test_fixture_conditions_robot_pairs(fresh_world):
    """The robot-pair fixture: an empty world list, at least 5 % of the rows decided by held-robot pairs."""
    arm, chain, obs = build_scene("c1")
    att, b = hc.reach_box(arm)
    sm, spec = arm.scene_model(), att.spec(arm)
    assert len(spec.world_shapes) == 0 and len(spec.robot_shapes) == 7
    q = sample_q(chain, 2000, seed=3)
    for thr in hc.THRESHOLDS:
        share = float(hc.held_mask(sm, spec, q, thr).mean())
        print(f"reach box thr={thr}: held-robot pairs collide in {share:.4f} of 2000 rows")
        assert 0.05 <= share <= 0.90, (thr, share)
