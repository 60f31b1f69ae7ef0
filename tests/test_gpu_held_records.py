"""Witness points and gradient rows of held items on the device (nbk_held_records_batch / nbk_held_records_items /
nbk_held_cloud_records_batch; DeviceModel.held_records / held_closest_records / held_cloud_records; Arm.attached_proximity_jacobians /
attached_closest_to / attached_cloud_proximity_jacobians / attached_cloud_closest_to; safe_sets.attached_distance_and_gradient).
Every field is bit for bit what the CPU oracle's ``proximity_jacobian`` gives on a descriptor that holds the held shapes as robot
shapes of the holding frame (tests/held_records_cases.py).  Needs a real MI355X.

The conditions the cases rely on -- items of both signs, rows that are not trivially zero, cloud cases with winners, losers and
several winning shapes -- are asserted on the REFERENCE before comparing, and pinned without a GPU by
tests/test_held_records_host.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from test_gpu_parity import torch_cuda      # noqa: F401  (fixture)
import held_cases as hc
import held_cloud_cases as hcc
import held_records_cases as rc
import held_traj_cases as tc

N = rc.N_ROWS


def _x(name):
    x = tc.scene(name)
    x.dev, x.held = x.att._device(x.arm)
    x.q = x.q[:N]
    return x


def _np(rec):
    return tuple(None if a is None else (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)) for a in rec)


# ---- 1. dense records --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c3", "c2", "c1"))
def test_dense_records(fresh_world, torch_cuda, name):
    torch = torch_cuda
    x = _x(name)
    q = x.q
    K = x.held.n_items
    ref = rc.item_ref(x, name, None)
    assert ref[0].shape == (N, K) and ref[1].shape == (N, K, 9) and ref[2].shape == (N, K, x.chain.dof)
    assert (ref[0] < 0.0).any() and (ref[0] > 0.0).any() and np.abs(ref[2]).max() > 0.1, "items of both signs, rows that are not zero"
    Gs = rc.grasps(x, name)
    refs = [rc.item_ref(x, name, k) for k in range(4)]
    pick = np.arange(N) % 4
    rows_ref = rc.per_row(refs, pick)
    poses = np.stack([Gs[k] for k in pick])
    for B in rc.BATCHES:
        got = x.dev.held_records(x.held, q[:B])
        assert all(isinstance(a, np.ndarray) for a in got)
        rc.assert_records(got, ref, f"{name} B={B}, the stored grasp", B)
        tc.assert_bits(got[0], x.dev.held_distances(x.held, q[:B]), f"{name} B={B}: the distances are held_distances'")
        rc.assert_records(x.dev.held_records(x.held, q[:B], pose=poses[:B]), rows_ref, f"{name} B={B}, a grasp per row", B)
    rc.assert_records(x.dev.held_records(x.held, q[:65], pose=Gs[1]), refs[1], f"{name}: one grasp for the call", 65)
    # the optional outputs
    d, w, j = x.dev.held_records(x.held, q[:65], witness=False)
    assert w is None
    rc.assert_records((d, ref[1][:65], j), ref, f"{name}: rows without witness", 65)
    d, w, j = x.dev.held_records(x.held, q[:65], jacobian=False)
    assert j is None
    rc.assert_records((d, w, ref[2][:65]), ref, f"{name}: witness without rows", 65)
    # device tensors stay on the device; the pose tensor is read in place
    qt, Gt = torch.from_numpy(q[:65]).cuda(), torch.from_numpy(Gs[2]).cuda()
    got = x.dev.held_records(x.held, qt, pose=Gt)
    assert all(a.is_cuda for a in got)
    rc.assert_records(got, refs[2], f"{name}: tensors", 65)
    # a NaN q row and a NaN grasp row: NaN in every field of that row only
    qb = q[:70].copy(); qb[3, 2] = np.nan; qb[66, 0] = np.inf
    got = x.dev.held_records(x.held, qb)
    assert rc.all_nan(got, [3, 66])
    keep = np.ones(70, dtype=bool); keep[[3, 66]] = False
    rc.assert_records([a[keep] for a in got], [r[:70][keep] for r in ref], f"{name}: the rows beside a NaN row")
    pb = poses[:70].copy(); pb[5, 1, 3] = np.nan
    got = x.dev.held_records(x.held, q[:70], pose=pb)
    assert rc.all_nan(got, [5])
    keep = np.ones(70, dtype=bool); keep[5] = False
    rc.assert_records([a[keep] for a in got], [r[:70][keep] for r in rows_ref], f"{name}: the rows beside a NaN grasp")


# ---- 2. listed records -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c3", "c1"))
def test_listed_records(fresh_world, torch_cuda, name):
    torch = torch_cuda
    x = _x(name)
    B, K = 70, x.held.n_items
    q = x.q[:B]
    rng = np.random.default_rng(12)
    out = np.array([[-1, 0], [B, 0], [0, K], [3, -1], [B + 5, K + 2]], dtype=np.int32)
    M = 300 + len(out)
    at = np.sort(rng.choice(M, len(out), replace=False))              # where the out-of-range entries stand among the 300
    inside = np.ones(M, dtype=bool); inside[at] = False
    items = np.zeros((M, 2), dtype=np.int32)
    items[inside] = np.stack((rng.integers(0, B, 300), rng.integers(0, K, 300)), axis=1)
    items[at] = out
    dense = x.dev.held_records(x.held, q)
    rc.assert_records(dense, rc.item_ref(x, name, None), f"{name}: dense", B)
    want = [a[items[inside, 0], items[inside, 1]] for a in dense]
    got = x.dev.held_records(x.held, q, items=items)
    assert got[0].shape == (M,) and got[1].shape == (M, 9) and got[2].shape == (M, x.chain.dof)
    rc.assert_records([a[inside] for a in got], want, f"{name}: listed against dense")
    assert rc.all_nan(got, at), "entries outside [0, B) x [0, K) are NaN in every field"
    # a grasp per row: a listed item takes the grasp of its own row; tensors in, tensors out
    Gs = rc.grasps(x, name)
    pick = np.arange(B) % 4
    poses = np.stack([Gs[k] for k in pick])
    dense = x.dev.held_records(x.held, q, pose=poses)
    rc.assert_records(dense, rc.per_row([rc.item_ref(x, name, k) for k in range(4)], pick), f"{name}: dense, a grasp per row", B)
    got = x.dev.held_records(x.held, torch.from_numpy(q).cuda(), pose=torch.from_numpy(poses).cuda(), items=torch.from_numpy(items).cuda())
    assert all(a.is_cuda for a in got)
    got = _np(got)
    rc.assert_records([a[inside] for a in got], [a[items[inside, 0], items[inside, 1]] for a in dense], f"{name}: listed, a grasp per row")
    assert rc.all_nan(got, at)
    # a NaN row of q: its listed entries are NaN, the others as they were
    qb = q.copy(); qb[int(items[inside][0, 0]), 1] = np.nan
    hit = inside & (items[:, 0] == items[inside][0, 0])
    got2 = x.dev.held_records(x.held, qb, items=items, pose=poses)
    assert rc.all_nan(got2, hit | ~inside)
    rc.assert_records([a[inside & ~hit] for a in got2], [a[inside & ~hit] for a in got], f"{name}: beside a NaN row")
    d, w, j = x.dev.held_records(x.held, q, items=items[:0])
    assert d.shape == (0,) and w.shape == (0, 9) and j.shape == (0, x.chain.dof)


# ---- 3. closest records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c3", "c1"))
def test_closest_records(fresh_world, torch_cuda, name):
    torch = torch_cuda
    from numbotics_amd.physics import Proximity
    from numbotics_amd.planning import safe_sets
    x = _x(name)
    q = x.q
    ref = rc.item_ref(x, name, None)
    cols = x.held.items()
    if name == "c1":
        assert (cols[:, 1] == 0).all(), "robot items only"
    dist, item = x.arm.attached_clearance(q, x.att)
    tc.assert_bits(dist, ref[0].min(axis=1), f"{name}: the clearance")
    assert np.array_equal(item, ref[0].argmin(axis=1))
    dense = x.dev.held_records(x.held, q)
    b = np.arange(N)
    want = (dist, dense[1][b, item], dense[2][b, item])
    d, it, w, j = x.dev.held_closest_records(x.held, q)
    assert it.dtype == np.int32 and np.array_equal(it, item)
    rc.assert_records((d, w, j), want, f"{name}: closest records")
    rc.assert_records((d, w, j), (ref[0][b, item], ref[1][b, item], ref[2][b, item]), f"{name}: closest records against the oracle")
    assert len(set(item.tolist())) >= 3, "several items are the closest somewhere"
    # the public entries: tensors stay on the device; per item; the IRIS form
    got = x.arm.attached_proximity_jacobians(torch.from_numpy(q).cuda().reshape(10, 13, -1), x.att)
    assert all(a.is_cuda for a in got) and got[0].shape == (N,)
    got = _np(got)
    assert np.array_equal(got[1], item)
    rc.assert_records((got[0], got[2], got[3]), want, f"{name}: attached_proximity_jacobians")
    rc.assert_records(x.arm.attached_proximity_jacobians(q, x.att, per_item=True), dense, f"{name}: per item")
    dg, jg = safe_sets.attached_distance_and_gradient(x.arm, q, x.att)
    rc.assert_records((dg, want[1], jg), want, f"{name}: attached_distance_and_gradient")
    # another grasp, and a row that is not finite
    G = rc.grasps(x, name)[3]
    refG = rc.item_ref(x, name, 3)
    iG = refG[0].argmin(axis=1)
    qb = q.copy(); qb[9, 0] = np.nan
    d, it, w, j = x.dev.held_closest_records(x.held, qb, pose=G)
    assert np.isnan(d[9]) and it[9] == -1 and np.isnan(w[9]).all() and np.isnan(j[9]).all()
    keep = b != 9
    assert np.array_equal(it[keep], iG[keep])
    rc.assert_records((d[keep], w[keep], j[keep]), (refG[0][b, iG][keep], refG[1][b, iG][keep], refG[2][b, iG][keep]), f"{name}: another grasp")
    assert x.arm.attached_closest_to(qb[9], x.att) is None
    # one configuration: a Proximity; for a robot item the link is the subject and the held object the target, for a world item the
    # held object is the subject and the obstacle the target
    kinds = cols[item, 1]
    names = x.att.items(x.arm)
    for kind in ((0, 1) if name == "c3" else (0,)):
        assert (kinds == kind).any(), f"{name}: no row whose closest item is of kind {kind}"
        r = int(np.flatnonzero(kinds == kind)[0])
        prox = x.arm.attached_closest_to(q[r], x.att)
        assert isinstance(prox, Proximity)
        if kind == 0:
            assert prox.subject is x.sm.links[x.sm.rshape_link[cols[item[r], 2]]] and prox.subject._name == names[item[r]][1]
            assert prox.target is x.att.objects[0]
        else:
            assert prox.subject is x.att.objects[0] and prox.target is x.sm.objects[x.sm.wshape_obj[cols[item[r], 2]]]
        tc.assert_bits(np.concatenate((prox.position_on_subject, prox.position_on_target, prox.normal_target_to_subject)), want[1][r], "Proximity")
        tc.assert_bits(np.float64(prox.distance), dist[r], "Proximity.distance")
    if name == "c3":
        # ties go to the smallest item: two copies of one box, standing in one place, make every item twice (their world copies are
        # new world shapes of the scene, so this comes last)
        from numbotics_amd.physics import Cuboid
        twin = [Cuboid(0.0, np.array(hc.BOX_HALF), collision_margin=hc.BOX_MARGIN, position=hc.PARK.copy()) for _ in range(2)]
        att2 = x.arm.attach(twin, "gripper", pose=hc.trans(0.0, 0.0, hc.BOX_Z))
        dev2, held2 = att2._device(x.arm)
        d2, i2, w2, j2 = dev2.held_closest_records(held2, q)
        cols2 = held2.items()
        assert cols2.shape[0] % 2 == 0 and set(cols2[:, 0].tolist()) == {0, 1} and (cols2[i2, 0] == 0).all(), "of two equal items the first"
        rc.assert_records((d2, w2, j2), want, "the twins' closest record is the one box's")
        # no items: inf, -1, NaN, rows of zeros
        from test_gpu_held import _spec, _device_held
        none = _device_held(x.dev, _spec(x.spec.frame, x.spec.A, x.spec.G, x.spec.shape_local, x.spec.shape_type, x.spec.shape_param, [], []))
        d0, i0, w0, j0 = x.dev.held_closest_records(none, q[:3])
        assert np.isposinf(d0).all() and (i0 == -1).all() and np.isnan(w0).all() and not j0.any() and j0.shape == (3, x.chain.dof)
        assert [a.shape for a in x.dev.held_records(none, q[:3])] == [(3, 0), (3, 0, 9), (3, 0, x.chain.dof)]


# ---- 4. other shape kinds ----------------------------------------------------------------------------------------------------------
def test_records_against_a_plane_and_hulls(fresh_world, torch_cuda):
    """The compound-mesh scene with a plane: a held box, sphere, capsule and cylinder against world hulls, a plane and a cube -- the
    EPA pass and, at B = 130, the hull's wave-uniform path."""
    from numbotics_amd.physics import Plane
    from numbotics_amd.scenes import build_scene, sample_q
    arm, chain, obs = build_scene("c5m")
    plane = Plane(0.0, np.array([0.0, 0.0, 1.0]), position=np.array([0.0, 0.0, 0.05]))
    q = sample_q(chain, 130, seed=3)
    bodies = hcc.kind_bodies()                   # (their parked world copies are world shapes of the scene: before scene_model())
    sm = arm.scene_model()
    kinds = {int(t) for t in sm.wshape_type}
    assert 5 in kinds and 4 in kinds and 2 in kinds, "hulls, the plane and the cube"
    signs = {5: set(), 4: set()}
    for kind, body in bodies.items():
        att = arm.attach(body, "gripper", pose=hc.trans(0.0, 0.0, hc.BOX_Z))
        spec = att.spec(arm)
        dev, held = att._device(arm)
        cols = held.items()
        ref = Oracle(hc.held_model(sm, spec)).proximity_jacobian(q)
        for B in (63, 130):                      # 63: every wave straddles items; 130: waves of one item, the hull's uniform path
            got = dev.held_records(held, q[:B])
            for k in range(cols.shape[0]):
                what = f"{kind} B={B} item {k} ({'world' if cols[k, 1] else 'robot'} {cols[k, 2]})"
                rc.assert_records([a[:, k] for a in got], [r[:B, k] for r in ref], what)
        wk = np.array([int(sm.wshape_type[c[2]]) if c[1] else -1 for c in cols])
        for t in (5, 4):
            sub = ref[0][:, wk == t]
            assert sub.size, f"{kind}: no item of world type {t}"
            signs[t] |= {bool((sub < 0.0).any()), 2 + bool((sub > 0.0).any())}
    assert signs[5] >= {True, 3} and signs[4] >= {True, 3}, "hull items and plane items of both signs"
    del plane, obs


# ---- 5. cloud records --------------------------------------------------------------------------------------------------------------
def _cloud(scan, **kw):
    from numbotics_amd.physics import PointCloud
    pts, r = hcc.scan(scan)
    return PointCloud(pts, r, **kw), pts, r


@pytest.mark.parametrize("per_shape", (False, True), ids=("per-configuration", "per-shape"))
@pytest.mark.parametrize("scan", ("dense", "sparse"))
def test_cloud_records(fresh_world, torch_cuda, scan, per_shape):
    torch = torch_cuda
    x = rc.eight_scene()
    dev, held = x.att._device(x.arm)
    cloud, pts, r = _cloud(scan)
    d_max = rc.D_MAX[scan]
    raw = rc.cloud_raw(x, scan)
    ref = rc.cloud_ref(x, raw, d_max, per_shape)
    one = rc.cloud_ref(x, raw, d_max, False)
    near = np.isfinite(one[0])
    assert near.sum() >= 10 and (~near).sum() >= 10 and len(set(one[1][near].tolist())) >= 3 and (one[0][near] < 0).any(), \
        "rows that win, rows that give inf, at least three winning held shapes, a penetrating record"
    nq = x.chain.dof
    for B in (1, 64, 65, N):
        got = dev.held_cloud_records(held, cloud, x.q[:B], d_max, per_shape=per_shape)
        assert got[0].shape == ((B, 8) if per_shape else (B,)) and got[4].shape == got[0].shape + (nq,)
        rc.assert_cloud_records(got, ref, f"{scan} per_shape={per_shape} B={B}", B)
    got = dev.held_cloud_records(held, cloud, x.q, d_max, per_shape=per_shape)
    # losers: +inf, -1, -1, a NaN witness and a row of +0.0 (the sign bit is clear)
    lose = np.isposinf(got[0])
    assert lose.any() and (got[1][lose] == -1).all() and (got[2][lose] == -1).all() and np.isnan(got[3][lose]).all()
    assert not got[4][lose].view(np.int64).any(), "a loser's row is +0.0"
    assert not np.isnan(got[3][~lose]).any()
    # dist, shape and point are held_cloud_clearance's
    if not per_shape:
        dc, sc, pc = dev.held_cloud_clearance(held, cloud, x.q, d_max)
        tc.assert_bits(got[0], dc, "distance against held_cloud_clearance")
        assert np.array_equal(got[1], sc) and np.array_equal(got[2], pc)
    # the optional outputs; tensors in, tensors out
    qt = torch.from_numpy(x.q).cuda()
    both = dev.held_cloud_records(held, cloud, qt, d_max, per_shape=per_shape)
    assert all(a.is_cuda for a in both)
    rc.assert_cloud_records(both, ref, "tensors")
    only_w = dev.held_cloud_records(held, cloud, x.q, d_max, per_shape=per_shape, jacobian=False)
    only_j = dev.held_cloud_records(held, cloud, x.q, d_max, per_shape=per_shape, witness=False)
    assert only_w[4] is None and only_j[3] is None
    rc.assert_cloud_records(only_w, ref, "witness without rows")
    rc.assert_cloud_records(only_j, ref, "rows without witness")
    # a NaN row of q, a NaN grasp row: NaN, -1, -1, NaN, NaN in that row only
    qb = x.q.copy(); qb[2, 1] = np.nan; qb[64, nq - 1] = np.inf
    got = dev.held_cloud_records(held, cloud, qb, d_max, per_shape=per_shape)
    for f in (0, 3, 4):
        assert np.isnan(got[f][[2, 64]]).all()
    assert (got[1][[2, 64]] == -1).all() and (got[2][[2, 64]] == -1).all()
    keep = np.ones(N, dtype=bool); keep[[2, 64]] = False
    rc.assert_cloud_records([a[keep] for a in got], [a[keep] for a in ref], "beside the NaN rows")
    poses = np.broadcast_to(x.spec.G, (N, 4, 4)).copy(); poses[7, 0, 3] = np.nan
    got = dev.held_cloud_records(held, cloud, x.q, d_max, pose=poses, per_shape=per_shape)
    assert np.isnan(got[0][7]).all() and (got[1][7] == -1).all() and np.isnan(got[3][7]).all() and np.isnan(got[4][7]).all()
    keep = np.arange(N) != 7
    rc.assert_cloud_records([a[keep] for a in got], [a[keep] for a in ref], "beside a NaN grasp row")
    # a set cloud status: NaN, -1, -1, NaN, NaN everywhere; an empty cloud: losers everywhere
    bad = pts.copy(); bad[5, 1] = np.inf
    sick, _, _ = _cloud(scan)
    sick.update(bad)
    assert sick.status() == 2
    got = dev.held_cloud_records(held, sick, x.q, d_max, per_shape=per_shape)
    assert np.isnan(got[0]).all() and (got[1] == -1).all() and (got[2] == -1).all() and np.isnan(got[3]).all() and np.isnan(got[4]).all()
    from numbotics_amd.physics import PointCloud
    empty = PointCloud(np.zeros((0, 3)), 0.01, bounds=([-1, -1, 0], [1, 1, 1]), capacity=8)
    got = dev.held_cloud_records(held, empty, x.q, d_max, per_shape=per_shape)
    assert np.isposinf(got[0]).all() and (got[1] == -1).all() and np.isnan(got[3]).all() and not got[4].view(np.int64).any()


def test_cloud_records_public_entries(fresh_world, torch_cuda):
    from numbotics_amd.physics import Proximity
    x = rc.eight_scene()
    dev, held = x.att._device(x.arm)
    cloud, pts, r = _cloud("dense")
    d_max = rc.D_MAX["dense"]
    raw = rc.cloud_raw(x, "dense")
    ref = rc.cloud_ref(x, raw, d_max, False)
    rc.assert_cloud_records(x.arm.attached_cloud_proximity_jacobians(x.q.reshape(10, 13, -1), x.att, cloud, d_max), ref, "per configuration")
    rc.assert_cloud_records(x.arm.attached_cloud_proximity_jacobians(x.q, x.att, cloud, d_max, per_shape=True),
                            rc.cloud_ref(x, raw, d_max, True), "per shape")
    # another grasp for the call: its own reference
    G = x.spec.G @ hc.rot_pose(np.random.default_rng(5), 0.3, 0.02) @ hc.trans(0, 0, -hc.BOX_Z)
    refG = rc.cloud_ref(x, rc.cloud_raw_of(x, pts, r, x.q[:65], G), d_max, False)
    assert np.isfinite(refG[0]).any() and refG[0].tobytes() != ref[0][:65].tobytes()
    rc.assert_cloud_records(dev.held_cloud_records(held, cloud, x.q[:65], d_max, pose=G), refG, "another grasp")
    near = np.isfinite(ref[0])
    b_near, b_far = int(np.flatnonzero(near)[0]), int(np.flatnonzero(~near)[0])
    prox = x.arm.attached_cloud_closest_to(x.q[b_near], x.att, cloud, d_max)
    assert isinstance(prox, Proximity) and prox.subject is x.att.objects[0] and prox.target is cloud
    tc.assert_bits(np.concatenate((prox.position_on_subject, prox.position_on_target, prox.normal_target_to_subject)), ref[3][b_near], "Proximity")
    tc.assert_bits(np.float64(prox.distance), ref[0][b_near], "Proximity.distance")
    assert x.arm.attached_cloud_closest_to(x.q[b_far], x.att, cloud, d_max) is None
    qn = x.q[b_near].copy(); qn[0] = np.nan
    assert x.arm.attached_cloud_closest_to(qn, x.att, cloud, d_max) is None


def test_cloud_update_and_records_in_one_graph(fresh_world, torch_cuda):
    """cloud.update -> held_cloud_records captured on one stream -- ONE records call in the graph -- with a static points tensor and
    a grasp tensor that is rewritten in place between the replays."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    import cloud_cases as cc
    x = rc.eight_scene()
    dev, held = x.att._device(x.arm)
    d_max, r = 0.1, 0.01
    sets = [np.ascontiguousarray(cc.scan(1000, seed=s)) for s in (0, 41, 42)]
    rng = np.random.default_rng(3)
    Gs = [x.spec.G @ hc.rot_pose(rng, 0.3, 0.02) @ hc.trans(0, 0, -hc.BOX_Z) for _ in range(3)]
    qt = torch.from_numpy(x.q).cuda()
    Pt = torch.from_numpy(sets[0]).cuda()
    Gt = torch.from_numpy(Gs[0].copy()).cuda()
    cloud = PointCloud(Pt, r, bounds=([-0.6, -0.6, 0.0], [0.6, 0.6, 1.0]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev.held_cloud_records(held, cloud, qt, d_max, pose=Gt)          # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cloud.update(Pt)
            rec = dev.held_cloud_records(held, cloud, qt, d_max, pose=Gt)
    torch.cuda.current_stream().wait_stream(side)
    seen = set()
    for k in (1, 2):
        Pt.copy_(torch.from_numpy(sets[k]).cuda())
        Gt.copy_(torch.from_numpy(Gs[k].copy()).cuda())
        graph.replay()
        torch.cuda.synchronize()
        got = _np(rec)
        ref = rc.cloud_ref(x, rc.cloud_raw_of(x, sets[k], r, x.q, Gs[k]), d_max, False)
        near = np.isfinite(ref[0])
        assert near.any() and not near.all(), f"replay {k}: not a mixed case"
        rc.assert_cloud_records(got, ref, f"replay {k}")
        seen.add(got[0].tobytes())
    assert len(seen) == 2, "the replays must differ"
    rc.assert_cloud_records(dev.held_cloud_records(held, cloud, x.q, d_max, pose=Gs[2]), got, "the eager call after the last replay")
    assert cloud.status() == 0
