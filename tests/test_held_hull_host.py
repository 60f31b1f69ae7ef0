"""Held meshes without a GPU: ``attach(..., meshes=True)`` resolves a Mesh to hull records with the tables a link mesh gets, the
refusal without the flag stays, the host twins of the motion bound with hull tables equal the scene's routine on the combined
descriptor, bad hull tables are refused, and -- by the oracle alone -- the fixtures of tests/held_hull_cases.py have what the GPU
tests (tests/test_gpu_held_hull.py) rely on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from numbotics_amd import _lib
from numbotics_amd.engine import edge_motion_bounds, spline_motion_bounds, held_edge_motion_bounds, held_spline_motion_bounds, model_desc
import held_cases as hc
import held_hull_cases as hh
import held_traj_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nbk_held_create_hulls", "nbk_edge_held_motion_bounds_hulls_host", "nbk_spline_held_motion_bounds_hulls_host")


def test_symbols_declared_and_bound():
    with open(os.path.join(ROOT, "include", "nbk.h")) as f:
        declared = set(re.findall(r"\b(nbk_\w+)\s*\(", f.read()))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/nbk.h"
        assert s in _lib.SYMBOLS, f"{s} is not listed in _lib.SYMBOLS"
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None
    a = np.zeros(12)
    out = C.c_void_p()
    assert lib.nbk_held_create_hulls(None, 0, a.ctypes.data, a.ctypes.data, 1, a.ctypes.data, a.ctypes.data, a.ctypes.data, 0, None, None,
                                     0, None, None, None, None, C.byref(out)) == -1


# ---- attach(..., meshes=True) --------------------------------------------------------------------------------------------------------
def test_attach_meshes_resolves_to_hull_records(fresh_world):
    """A held Mesh becomes NBK_HULL records whose tables are what the same mesh gives as a link shape (``_shape_records`` with a
    ``HullTable``): one hull, one per file object with convex_decomposition, Bullet's 0.001 margin in the default shape mode."""
    from numbotics_amd.physics import Mesh, Cuboid
    from numbotics_amd.robots.model import HullTable, _shape_records, SH_HULL, SH_BOX
    from numbotics_amd.scenes import build_scene
    arm, chain, obs = build_scene("c2")
    rock = Mesh(0.0, hh.mesh_path("rock.obj"), position=hc.PARK.copy())
    att = arm.attach(rock, "gripper", pose=hh.GRASP["rock"], meshes=True)
    spec = att.spec(arm)
    table = HullTable()
    recs = _shape_records(rock._collision_shape, np.eye(4), table, True)
    vb, hv, fb, hp = table.arrays()
    assert spec.n_shapes == len(recs) == 1 and spec.n_hulls == 1 and int(spec.shape_type[0]) == SH_HULL == 5
    assert np.array_equal(spec.hull_vert_begin, vb) and np.array_equal(spec.hull_face_begin, fb)
    tc.assert_bits(spec.hull_verts, hv, "hull vertices")
    tc.assert_bits(spec.hull_planes, hp, "hull planes")
    tc.assert_bits(spec.shape_local[0], recs[0][1], "the hull's local pose")
    tc.assert_bits(spec.shape_param[0], recs[0][2], "the hull's parameters")
    assert spec.shape_param[0][0] == 0.0 and spec.shape_param[0][3] == 0.001
    assert att.has_mesh and spec.hulls is not None
    # the sharp shape mode: no margin
    arm0, chain0, obs0 = build_scene("c2", bullet_margins=False)
    assert arm0.attach(rock, "gripper", pose=hh.GRASP["rock"], meshes=True).spec(arm0).shape_param[0][3] == 0.0
    # one hull per file object with convex_decomposition; a box between two meshes: hull, box, hull with hull indices 0 and 1
    table_obj = Mesh(0.0, hh.mesh_path("table.obj"), convex_decomposition=True, position=hc.PARK.copy())
    sp5 = arm.attach(table_obj, "gripper", pose=np.eye(4), meshes=True).spec(arm)
    assert sp5.n_shapes == 5 and sp5.n_hulls == 5 and [int(p[0]) for p in sp5.shape_param] == [0, 1, 2, 3, 4]
    spec3, att3, keep = hh.fixture(arm, "mixed")
    assert [int(t) for t in spec3.shape_type] == [SH_HULL, SH_BOX, SH_HULL] and spec3.n_hulls == 2
    assert spec3.shape_param[0][0] == 0.0 and spec3.shape_param[2][0] == 1.0
    # the total still counts against 8
    with pytest.raises(ValueError, match="at most 8"):
        arm.attach([table_obj, Mesh(0.0, hh.mesh_path("table.obj"), convex_decomposition=True, position=hc.PARK.copy())], "gripper",
                   pose=np.eye(4), meshes=True)
    # a primitive attachment has no hull tables, with or without the flag
    b = Cuboid(0.0, np.array([0.1, 0.1, 0.1]), position=hc.PARK.copy())
    for flag in (False, True):
        a = arm.attach(b, "gripper", pose=np.eye(4), meshes=flag)
        assert a.spec(arm).hulls is None and a.spec(arm).n_hulls == 0 and not a.has_mesh


def test_refusals_stay(fresh_world):
    from numbotics_amd.physics import Mesh, Plane
    from numbotics_amd.physics.attachment import HeldSpec
    from numbotics_amd.scenes import build_scene
    arm, chain, obs = build_scene("c2")
    rock = Mesh(0.0, hh.mesh_path("rock.obj"), position=hc.PARK.copy())
    with pytest.raises(ValueError, match="MESH") as e:
        arm.attach(rock, "gripper", pose=np.eye(4))
    assert "pass meshes=True" in str(e.value)
    pl = Plane(0.0, np.array([0.0, 0.0, 1.0]), position=hc.PARK.copy())
    for flag in (False, True):
        with pytest.raises(ValueError, match="PLANE"):
            arm.attach(pl, "gripper", pose=np.eye(4), meshes=flag)
    # HeldSpec without the hull fields: none
    sp = HeldSpec(frame=0, A=np.eye(4), G=np.eye(4), shape_local=np.eye(4)[None], shape_type=np.array([2], dtype=np.int32),
                  shape_param=np.array([[0.1, 0.1, 0.1, 0.0]]), world_shapes=np.zeros(0, dtype=np.int32), robot_shapes=np.zeros(0, dtype=np.int32))
    assert sp.n_hulls == 0 and sp.hulls is None
    # the connectors refuse a held mesh that is to see a scan, before a cloud is looked at
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector
    att = arm.attach(rock, "gripper", pose=hh.GRASP["rock"], meshes=True)
    with pytest.raises(ValueError, match="held meshes do not see scans yet"):
        ConnectorParams(arm=arm, cloud=object(), attached=att, attached_sees_cloud=True)
    with pytest.raises(ValueError, match="held meshes do not see scans yet"):
        ContinuousConnector(ConnectorParams(arm=arm), cloud=object(), attached=att, attached_sees_cloud=True)


# ---- the motion bound ----------------------------------------------------------------------------------------------------------------
def _tree():
    from continuous_ref import tree_scene, random_edges
    import types
    arm, chain, obs = tree_scene()
    spec, probe = hh.hull_spec(arm, 0.3 * hh.TETRA, hc.trans(0.0, 0.01, 0.06), link="tip_b",
                               extra=((hc.SH_BOX, hc.trans(0.0, 0.0, 0.05), (0.02, 0.03, 0.05, 0.004)),
                                      (hh.SH_HULL, hc.trans(0.01, 0.0, -0.02), 0.2 * hh.FLAT)))
    return types.SimpleNamespace(arm=arm, chain=chain, keep=(obs, probe), sm=arm.scene_model(), spec=spec,
                                 q=random_edges(chain, 2000, 3)[0])


@pytest.mark.parametrize("name", ("kinova", "tree"))
def test_motion_bounds_equal_the_scene_routine(fresh_world, name):
    """The *_hulls_host twins give, item by item, the bits ``edge_motion_bounds`` / ``spline_motion_bounds`` give for the held pairs
    of the combined descriptor, with the stored grasp and with another: on the Kinova arm (the mixed attachment: hull, box, hull)
    and on the tree with a prismatic joint below a revolute one."""
    x = _tree() if name == "tree" else hh.scene("c2", "mixed")
    K = len(tc.item_columns(x.sm, x.spec))
    assert K > 0 and (np.asarray(x.spec.shape_type) == hh.SH_HULL).sum() == 2
    if name == "tree":
        kin = x.sm.kin
        path, f = [], x.spec.frame
        while f >= 0:
            path.append(int(f))
            f = int(kin.joint_parent[f])
        types_ = [int(kin.joint_type[j]) for j in path[::-1]]
        assert 1 in types_[1:] and 0 in types_[:types_.index(1, 1)], f"a prismatic joint below a revolute one on the holding path: {types_}"
    s, g = tc.edges(x, 40)
    rng = np.random.default_rng(11)
    for G in (None, x.spec.G @ hc.rot_pose(rng, 0.4, 0.03)):
        hm = hh.held_model_hulls(x.sm, x.spec, G)
        assert hm.n_pairs == K and hm.n_hulls == x.sm.n_hulls + 2
        ref = edge_motion_bounds(hm, s, g)
        got = held_edge_motion_bounds(x.sm, x.spec, s, g, G=G)
        assert (ref > 0.0).all()
        tc.assert_bits(got, ref, f"{name} edge mu")
        both = edge_motion_bounds(hh.held_model_hulls(x.sm, x.spec, G, keep_scene=True), s, g)
        tc.assert_bits(both[:, x.sm.n_pairs:], ref, f"{name} edge mu, combined model")
        for degree in (1, 3):
            ctrl, knots = tc.splines(x, degree, S=12)
            knots = knots.copy()
            if degree == 3:
                knots[4] = knots[3]                       # an empty span: its entries are 0
            ref = spline_motion_bounds(hm, ctrl, knots, degree)
            got = held_spline_motion_bounds(x.sm, x.spec, ctrl, knots, degree, G=G)
            tc.assert_bits(got, ref, f"{name} spline mu, degree {degree}")
            assert (ref > 0.0).any()
    # the hull's bound radius enters: a hull scaled up has larger bounds
    import dataclasses
    small, _ = hh.hull_spec(x.arm, 0.3 * hh.TETRA, x.spec.G, link="tip_b" if name == "tree" else "gripper")
    planes = small.hull_planes.copy(); planes[:, 3] *= 10.0
    big = dataclasses.replace(small, hull_verts=10.0 * small.hull_verts, hull_planes=planes)
    sm = x.arm.scene_model()
    assert (held_edge_motion_bounds(sm, big, s, g) > held_edge_motion_bounds(sm, small, s, g)).all()


# ---- bad tables --------------------------------------------------------------------------------------------------------------------
def test_bad_hull_tables_are_invalid(fresh_world):
    """The checks nbk_model_create gives a descriptor's hulls, through the host twin (the creator shares them, and needs a device):
    a plane that cuts off a vertex, a non-unit normal, a hull index out of range, a table that does not start at 0, an empty hull --
    NBK_ERR_INVALID each; the twins without tables keep answering NBK_ERR_UNSUPPORTED."""
    from numbotics_amd.engine import _held_host_args, _held_hull_args
    x = hh.scene("c2", "tetra")
    s, g = tc.edges(x, 4)
    d, keep = model_desc(x.sm)
    lib = _lib.load()
    args, keep2, K = _held_host_args(x.sm, x.spec, None)
    mu = np.zeros((4, K))

    def call(spec, sp=None):
        a, k2, _ = _held_host_args(x.sm, spec if sp is None else sp, None)
        h, k3 = _held_hull_args((spec.hull_vert_begin, spec.hull_verts, spec.hull_face_begin, spec.hull_planes))
        return lib.nbk_edge_held_motion_bounds_hulls_host(C.byref(d), *a, *h, s.ctypes.data, g.ctypes.data, 4, mu.ctypes.data)

    import dataclasses
    assert call(x.spec) == 0
    assert lib.nbk_edge_held_motion_bounds_host(C.byref(d), *args, s.ctypes.data, g.ctypes.data, 4, mu.ctypes.data) == -4
    P = x.spec.hull_planes.copy()
    assert P.shape == (4, 4)
    cut = P.copy(); cut[1, 3] -= 0.05                     # the plane moves inwards: a vertex lies outside it
    assert call(dataclasses.replace(x.spec, hull_planes=cut)) == -1
    long = P.copy(); long[2, :3] *= 1.001                 # a normal that is not of unit length
    assert call(dataclasses.replace(x.spec, hull_planes=long)) == -1
    for idx in (1.0, -1.0, 0.5):                          # a hull index out of range, or no index
        sp = x.spec.shape_param.copy(); sp[0, 0] = idx
        assert call(dataclasses.replace(x.spec, shape_param=sp)) == -1
    assert call(dataclasses.replace(x.spec, hull_vert_begin=np.array([1, 4], dtype=np.int32))) == -1
    assert call(dataclasses.replace(x.spec, hull_vert_begin=np.array([0, 0], dtype=np.int32), hull_verts=np.zeros((0, 3)))) == -1
    nanv = x.spec.hull_verts.copy(); nanv[2, 1] = np.nan
    assert call(dataclasses.replace(x.spec, hull_verts=nanv)) == -1
    # no tables at all, and a hull shape: its index has nothing to name
    none = np.zeros(1, dtype=np.int32)
    assert lib.nbk_edge_held_motion_bounds_hulls_host(C.byref(d), *args, 0, none.ctypes.data, None, none.ctypes.data, None, s.ctypes.data,
                                                      g.ctypes.data, 4, mu.ctypes.data) == -1
    # the spline twin shares the rule
    ctrl, knots = tc.splines(x, 3, S=2)
    h, k3 = _held_hull_args((x.spec.hull_vert_begin, x.spec.hull_verts, x.spec.hull_face_begin, cut))
    out = np.zeros((2, 3, K))
    assert lib.nbk_spline_held_motion_bounds_hulls_host(C.byref(d), *args, *h, ctrl.ctypes.data, 2, 6, 3, knots.ctypes.data,
                                                        out.ctypes.data) == -1
    del keep, keep2


# ---- what the GPU tests rely on, by the oracle alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c2", "c5m"))
@pytest.mark.parametrize("kind", hh.FIXTURES)
def test_fixture_conditions(fresh_world, name, kind):
    from oracle.cpu_oracle import Oracle
    x = hh.scene(name, kind)
    assert (np.asarray(x.spec.shape_type) == hh.SH_HULL).any()
    if kind == "flat":
        assert x.spec.hull_planes.shape[0] == 0, "the flat hull has no planes"
    if kind == "tetra":
        assert x.spec.hull_verts.shape[0] == 4
    if kind == "mixed":
        assert [int(t) for t in x.spec.shape_type] == [5, 2, 5]
    pairs = hh.sphere_hull_items(x.sm, x.spec)
    for thr in hh.THRESHOLDS:
        ref = hh.held_mask(x.sm, x.spec, x.q, thr)
        assert 0.05 <= ref.mean() <= 0.95, f"{name} {kind} thr={thr}: {ref.mean():.3f} of the rows collide"
        both = Oracle(hh.held_model_hulls(x.sm, x.spec, keep_scene=True)).validity(x.q, thr, nthreads=8)
        own = Oracle(x.sm).validity(x.q, thr, nthreads=8)
        assert (both & ~own).sum() >= 5, "the held object must decide rows the scene lets through"
        # the known deviation (hull_box_far at tc <= 0 against a point core): no such item at a threshold where it could show
        assert all((thr + ma) + mb > 0.0 for ma, mb in pairs), f"{name} {kind} thr={thr}: a sphere-versus-held-hull item at tc <= 0"
