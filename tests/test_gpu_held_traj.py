"""Held objects on trajectories, on the device: item distances (nbk_held_distances_batch, Arm.attached_clearance), certified edges and
splines (nbk_edge_held_continuous_batch, nbk_spline_held_continuous_batch), sampled splines (nbk_spline_held_validity_batch) and the
connectors that use them -- every result bit for bit the CPU reference's on ``held_cases.held_model`` (tests/held_traj_cases.py).
Needs a real MI355X.

The shares of FREE / COLLISION / UNDECIDED trajectories of every fixture are pinned without a GPU by tests/test_held_traj_host.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from test_gpu_parity import torch_cuda      # noqa: F401  (fixture)
from ca_ref import FREE, COLLISION, UNDECIDED, DEGENERATE
import held_cases as hc
import held_traj_cases as tc


def _x(name):
    x = tc.scene(name)
    x.dev, x.held = x.att._device(x.arm)
    return x


def _same(got, ref, what, names):
    for a, r, n in zip(got, ref, names):
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        if r.dtype == bool:
            a = a.astype(bool)
        tc.assert_bits(a, r, f"{what}: {n}")


CERT = ("valid", "end", "t_free", "status")
SPL = ("valid", "t_free", "status")
SMP = ("valid", "t_hit", "n_samples")


# ---- 1. distances ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c3", "c2", "c1"))
def test_held_distances(fresh_world, torch_cuda, name):
    torch = torch_cuda
    x = _x(name)
    cols = tc.item_columns(x.sm, x.spec)
    K = len(cols)
    assert x.held.n_items == K and np.array_equal(x.held.items(), cols)
    q = x.q[:1000]
    ref = Oracle(hc.held_model(x.sm, x.spec)).pair_distances(q)
    assert ref.shape == (1000, K) and (ref < 0.0).any() and (ref > 0.0).any()
    rng = np.random.default_rng(21)
    Gs = [hc.rot_pose(rng) if name == "c3" else x.spec.G @ hc.rot_pose(rng, 0.3, 0.02) @ hc.trans(0, 0, -hc.BOX_Z) for _ in range(4)]
    refs = [Oracle(hc.held_model(x.sm, x.spec, G)).pair_distances(q) for G in Gs]
    pick = np.arange(1000) % 4
    per_row = np.stack([refs[pick[b]][b] for b in range(1000)])
    poses = np.stack([Gs[k] for k in pick])
    for B in tc.BATCHES:
        got = x.dev.held_distances(x.held, q[:B])
        assert isinstance(got, np.ndarray)
        tc.assert_bits(got, ref[:B], f"{name} B={B}, the stored grasp")
        tc.assert_bits(x.dev.held_distances(x.held, q[:B], pose=poses[:B]), per_row[:B], f"{name} B={B}, a grasp per row")
    tc.assert_bits(x.dev.held_distances(x.held, q[:65], pose=Gs[1]), refs[1][:65], f"{name}: one grasp for the call")
    # device tensors stay on the device; the pose tensor is read in place
    qt, Gt = torch.from_numpy(q[:65]).cuda(), torch.from_numpy(Gs[2]).cuda()
    dt = x.dev.held_distances(x.held, qt, pose=Gt)
    assert dt.is_cuda
    tc.assert_bits(dt.cpu().numpy(), refs[2][:65], f"{name}: tensors")
    # rows that are not finite
    qb = q[:70].copy(); qb[3, 2] = np.nan; qb[66, 0] = np.inf
    got = x.dev.held_distances(x.held, qb)
    assert np.isnan(got[[3, 66]]).all()
    keep = np.ones(70, dtype=bool); keep[[3, 66]] = False
    tc.assert_bits(got[keep], ref[:70][keep], f"{name}: the rows beside a NaN row")
    pb = poses[:70].copy(); pb[5, 1, 3] = np.nan
    got = x.dev.held_distances(x.held, q[:70], pose=pb)
    assert np.isnan(got[5]).all()
    keep = np.ones(70, dtype=bool); keep[5] = False
    tc.assert_bits(got[keep], per_row[:70][keep], f"{name}: the rows beside a NaN grasp")


def test_attached_clearance(fresh_world, torch_cuda):
    torch = torch_cuda
    x = _x("c3")
    q = x.q[:200]
    ref = Oracle(hc.held_model(x.sm, x.spec)).pair_distances(q)
    dist, item = x.arm.attached_clearance(q, x.att)
    assert dist.shape == item.shape == (200,)
    tc.assert_bits(dist, ref.min(axis=1), "clearance")
    assert np.array_equal(item, ref.argmin(axis=1))
    assert len(set(item.tolist())) >= 4, "several items are the closest somewhere"
    names = x.att.items(x.arm)
    assert len(names) == ref.shape[1]
    d0, i0 = x.arm.attached_clearance(q[7], x.att)
    assert isinstance(d0, float) and isinstance(i0, int) and d0 == ref[7].min() and i0 == int(ref[7].argmin())
    # on the device, and another grasp
    G = hc.rot_pose(np.random.default_rng(2))
    refG = Oracle(hc.held_model(x.sm, x.spec, G)).pair_distances(q)
    dt, it = x.arm.attached_clearance(torch.from_numpy(q).cuda(), x.att, pose=G)
    assert dt.is_cuda and it.is_cuda
    tc.assert_bits(dt.cpu().numpy(), refG.min(axis=1), "clearance, another grasp")
    assert np.array_equal(it.cpu().numpy(), refG.argmin(axis=1))
    qb = q[:5].copy(); qb[1, 0] = np.nan
    db, ib = x.arm.attached_clearance(qb, x.att)
    assert np.isnan(db[1]) and ib[1] == -1 and db[0] == ref[0].min()
    # ties go to the smallest item: two copies of one box, standing in one place, make every item twice (their world copies are
    # new world shapes of the scene, so this comes last)
    from numbotics_amd.physics import Cuboid
    twin = [Cuboid(0.0, np.array(hc.BOX_HALF), collision_margin=hc.BOX_MARGIN, position=hc.PARK.copy()) for _ in range(2)]
    att2 = x.arm.attach(twin, "gripper", pose=hc.trans(0.0, 0.0, hc.BOX_Z))
    d2, i2 = x.arm.attached_clearance(q, att2)
    cols = att2._device(x.arm)[1].items()
    assert cols.shape[0] % 2 == 0 and set(cols[:, 0].tolist()) == {0, 1} and (cols[i2, 0] == 0).all(), "of two equal items the first"
    tc.assert_bits(d2, ref.min(axis=1), "the twins' clearance is the one box's")


def test_held_distances_to_a_plane_and_hulls(fresh_world, torch_cuda):
    """The compound-mesh scene with a plane: a held box, sphere, capsule and cylinder against world hulls, a plane and a cube."""
    from numbotics_amd.physics import Plane, Sphere, Capsule, Cylinder, Cuboid
    from numbotics_amd.scenes import build_scene, sample_q
    arm, chain, obs = build_scene("c5m")
    plane = Plane(0.0, np.array([0.0, 0.0, 1.0]), position=np.array([0.0, 0.0, 0.05]))
    q = sample_q(chain, 130, seed=3)
    bodies = {"box": Cuboid(0.0, np.array([0.08, 0.1, 0.18]), position=hc.PARK.copy()),
              "sphere": Sphere(0.0, 0.2, position=hc.PARK.copy()),
              "capsule": Capsule(0.0, 0.08, 0.4, position=hc.PARK.copy()),
              "cylinder": Cylinder(0.0, 0.12, 0.4, position=hc.PARK.copy())}
    sm = arm.scene_model()
    kinds = {int(t) for t in sm.wshape_type}
    assert 5 in kinds and 4 in kinds and 2 in kinds, "hulls, the plane and the cube"
    signs = {5: set(), 4: set()}
    for kind, body in bodies.items():
        att = arm.attach(body, "gripper", pose=hc.trans(0.0, 0.0, hc.BOX_Z))
        spec = att.spec(arm)
        dev, held = att._device(arm)
        cols = held.items()
        ref = Oracle(hc.held_model(sm, spec)).pair_distances(q)
        for B in (63, 130):                      # 63: every wave straddles items; 130: waves of one item, the hull's uniform path
            got = dev.held_distances(held, q[:B])
            for k in range(cols.shape[0]):
                what = f"{kind} B={B} item {k} ({'world' if cols[k, 1] else 'robot'} {cols[k, 2]})"
                tc.assert_bits(got[:, k], ref[:B, k], what)
        wk = np.array([int(sm.wshape_type[c[2]]) if c[1] else -1 for c in cols])
        for t in (5, 4):
            sub = ref[:, wk == t]
            assert sub.size, f"{kind}: no item of world type {t}"
            signs[t] |= {bool((sub < 0.0).any()), 2 + bool((sub > 0.0).any())}
    assert signs[5] >= {True, 3} and signs[4] >= {True, 3}, "hull items and plane items of both signs"
    del plane, obs


# ---- 2. certified edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", (0.0, 0.01))
@pytest.mark.parametrize("mode", ("connect", "steer"))
@pytest.mark.parametrize("name", ("c3", "c2", "c1"))
def test_certified_edges(fresh_world, torch_cuda, name, mode, thr):
    x = _x(name)
    s, g = tc.edges(x)
    maxd = tc.MAXD if mode == "connect" else tc.MAXD_STEER
    ref = tc.edge_ref(x, name, False, mode, thr)
    free, col, und = tc.shares(ref[3])
    assert min(free, col, und) >= 3, (free, col, und)
    for E in tc.EDGE_COUNTS:
        got = x.dev.held_edge_continuous(x.held, s[:E], g[:E], maxd, mode=mode, threshold=thr)
        _same(got, tuple(a[:E] for a in ref), f"{name} {mode} thr={thr} E={E}", CERT)


def test_certified_edges_special_rows(fresh_world, torch_cuda):
    """max_iter = 3, a degenerate edge, a NaN configuration, given lengths, another grasp, a grasp that is not finite, no items."""
    from continuous_ref import reference_continuous
    x = _x("c3")
    hm = hc.held_model(x.sm, x.spec)
    orc = Oracle(hm)
    s, g = tc.edges(x, 65)
    ref = tc.edge_ref(x, "c3", False, "connect", 0.0, max_iter=3, E=65)
    assert (ref[3] == UNDECIDED).sum() > tc.shares(tc.edge_ref(x, "c3", E=65)[3])[2], "items stopped by exhaustion"
    _same(x.dev.held_edge_continuous(x.held, s, g, tc.MAXD, max_iter=3), ref, "max_iter=3", CERT)
    s2, g2 = s.copy(), g.copy()
    g2[4] = s2[4]                                   # degenerate
    ref = reference_continuous(hm, orc, s2, g2, tc.MAXD)[:4]
    assert ref[3][4] == DEGENERATE and np.isnan(ref[1][4]).all()
    _same(x.dev.held_edge_continuous(x.held, s2, g2, tc.MAXD), ref, "a degenerate edge", CERT)
    # a NaN configuration: the edge's length is NaN, which makes it degenerate (the reference's exact norm does not take a NaN: the
    # other rows are compared, and this one is stated)
    s2[9, 3] = np.nan
    got = x.dev.held_edge_continuous(x.held, s2, g2, tc.MAXD)
    assert got[3][9] == DEGENERATE and not got[0][9] and np.isnan(got[2][9]) and np.isnan(got[1][9]).all()
    rest = np.arange(65) != 9
    _same(tuple(a[rest] for a in got), tuple(a[rest] for a in ref), "beside a NaN row", CERT)
    # ... and with a length of its own it is UNDECIDED at t = 0, as against a cloud: q(t) is not finite, no distance is evaluated
    dist = np.linalg.norm(g - s, axis=1) * 1.25
    dist[4] = 0.5
    ref = reference_continuous(hm, orc, s, g2, 0.5, mode="steer", dist=dist)[:4]
    assert ref[3][4] != DEGENERATE and min(tc.shares(ref[3])) >= 3
    got = x.dev.held_edge_continuous(x.held, s2, g2, 0.5, mode="steer", dist=dist)
    assert got[3][9] == UNDECIDED and got[2][9] == 0.0 and not got[0][9]
    _same(tuple(a[rest] for a in got), tuple(a[rest] for a in ref), "given lengths", CERT)
    G = hc.rot_pose(np.random.default_rng(4))
    hmG = hc.held_model(x.sm, x.spec, G)
    ref = reference_continuous(hmG, Oracle(hmG), s, g, tc.MAXD)[:4]
    assert min(tc.shares(ref[3])) >= 3
    _same(x.dev.held_edge_continuous(x.held, s, g, tc.MAXD, pose=G), ref, "another grasp", CERT)
    bad = G.copy(); bad[2, 1] = np.inf
    valid, end, t_free, st = x.dev.held_edge_continuous(x.held, s2, g2, tc.MAXD, pose=bad)
    live = np.ones(65, dtype=bool); live[[4, 9]] = False
    assert not valid.any() and np.isnan(t_free).all()
    assert (st[live] == UNDECIDED).all() and (st[~live] == DEGENERATE).all()
    tc.assert_bits(end[rest], reference_continuous(hm, orc, s, g2, tc.MAXD)[1][rest], "end states do not depend on the grasp")
    assert np.isnan(end[9]).all()
    # no items: every non-degenerate edge is FREE at T_f
    from test_gpu_held import _spec, _device_held
    none = _device_held(x.dev, _spec(x.spec.frame, x.spec.A, x.spec.G, x.spec.shape_local, x.spec.shape_type, x.spec.shape_param, [], []))
    assert none.n_items == 0 and x.dev.held_distances(none, x.q[:3]).shape == (3, 0)
    valid, end, t_free, st = x.dev.held_edge_continuous(none, s2, g2, 0.5, mode="steer")
    assert (st[live] == FREE).all() and valid[live].all() and (st[~live] == DEGENERATE).all()
    d = np.linalg.norm(g2[live] - s2[live], axis=1)
    assert np.array_equal(t_free[live] < 1.0, d > 0.5) and (t_free[live] < 1.0).any()


@pytest.mark.parametrize("name", ("c3", "c1"))
def test_certified_edges_accumulate(fresh_world, torch_cuda, name):
    """edge_continuous, then held_edge_continuous(out=): the reference on the combined model."""
    torch = torch_cuda
    x = _x(name)
    s, g = tc.edges(x)
    ref = tc.edge_ref(x, name, True)
    only = tc.edge_ref(x, name, False)
    assert ((ref[3] != FREE) & (only[3] == FREE)).sum() >= 1 and ((ref[3] != FREE) & (only[3] != FREE)).sum() >= 3
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    for E in (65, 130):
        res = x.dev.edge_continuous(st[:E], gt[:E], tc.MAXD)
        scene_status = res[3].cpu().numpy().copy()
        out = x.dev.held_edge_continuous(x.held, st[:E], gt[:E], tc.MAXD, out=(res[0], res[2], res[3]))
        assert out[0] is res[0] and out[2] is res[2] and out[3] is res[3]
        _same((res[0], out[1], res[2], res[3]), tuple(a[:E] for a in ref), f"{name} accumulated E={E}", CERT)
        if name == "c3":
            assert ((scene_status == FREE) & (ref[3][:E] != FREE)).sum() >= 5, "the held box stops edges the scene lets through"


def test_certified_edges_capture(fresh_world, torch_cuda):
    """One captured graph, the grasp tensor rewritten between two replays (the second time with a value that is not finite)."""
    torch = torch_cuda
    from continuous_ref import reference_continuous
    x = _x("c3")
    E = 65
    s, g = tc.edges(x, E)
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    rng = np.random.default_rng(9)
    Gs = [hc.rot_pose(rng) for _ in range(3)]
    Gt = torch.from_numpy(Gs[0].copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x.dev.held_edge_continuous(x.held, st, gt, tc.MAXD, pose=Gt)                   # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            res = x.dev.edge_continuous(st, gt, tc.MAXD)
            x.dev.held_edge_continuous(x.held, st, gt, tc.MAXD, pose=Gt, out=(res[0], res[2], res[3]))
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for k in (1, 2):
        Gt.copy_(torch.from_numpy(Gs[k].copy()).cuda())
        graph.replay()
        torch.cuda.synchronize()
        hm = hc.held_model(x.sm, x.spec, Gs[k], keep_scene=True)
        ref = reference_continuous(hm, Oracle(hm), s, g, tc.MAXD)
        _same((res[0], res[2], res[3]), (ref[0], ref[2], ref[3]), f"replay {k}", SPL)
        seen.append(ref[3].tobytes() + ref[2].tobytes())
    assert seen[0] != seen[1]
    bad = Gs[2].copy(); bad[0, 3] = np.nan
    Gt.copy_(torch.from_numpy(bad).cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert not res[0].cpu().numpy().any() and np.isnan(res[2].cpu().numpy()).all() and (res[3].cpu().numpy() == UNDECIDED).all()
    # the entry point on a capturing stream, at the C boundary: graph nodes only, no allocation
    from numbotics_amd import _lib
    lib = _lib.load()
    v = torch.zeros((E,), dtype=torch.uint8, device="cuda")
    tf = torch.zeros((E,), dtype=torch.float64, device="cuda")
    stt = torch.zeros((E,), dtype=torch.int32, device="cuda")
    Gt.copy_(torch.from_numpy(Gs[1].copy()).cuda())
    with torch.cuda.stream(side):
        sp = C.c_void_p(side.cuda_stream)
        g3 = torch.cuda.CUDAGraph()
        g3.capture_begin()
        assert lib.nbk_edge_held_continuous_batch(x.dev._h, x.held._h, st.data_ptr(), gt.data_ptr(), None, E, tc.MAXD, 0, 0.0, 64, 1e-6,
                                                  Gt.data_ptr(), 0, v.data_ptr(), None, tf.data_ptr(), stt.data_ptr(), sp) == 0
        assert lib.nbk_edge_held_continuous_batch(x.dev._h, x.held._h, st.data_ptr(), gt.data_ptr(), None, E, tc.MAXD, 0, 0.0, 0, 1e-6,
                                                  Gt.data_ptr(), 0, v.data_ptr(), None, tf.data_ptr(), stt.data_ptr(), sp) == -1
        g3.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    g3.replay()
    torch.cuda.synchronize()
    hm = hc.held_model(x.sm, x.spec, Gs[1])
    ref = reference_continuous(hm, Oracle(hm), s, g, tc.MAXD)
    _same((v, tf, stt), (ref[0], ref[2], ref[3]), "captured at the C boundary", SPL)


# ---- 3. certified splines ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", (1, 2, 3, 4, 5))
def test_certified_splines(fresh_world, torch_cuda, degree):
    torch = torch_cuda
    x = _x("c3")
    ctrl, knots = tc.splines(x, degree)
    ref = tc.spline_ref(x, "c3", False, degree)
    assert 0 < (ref[2] == FREE).sum() < tc.N_SPLINES
    for S in tc.SPLINE_COUNTS:
        got = x.dev.held_spline_continuous(x.held, ctrl[:S], knots, degree)
        _same(got, tuple(a[:S] for a in ref), f"degree {degree} S={S}", SPL)
    # accumulated into the scene's result: the reference on the combined model
    both = tc.spline_ref(x, "c3", True, degree)
    ct = torch.from_numpy(ctrl).cuda()
    res = x.dev.spline_continuous(ct, knots, degree)
    assert x.dev.held_spline_continuous(x.held, ct, knots, degree, out=res)[0] is res[0]
    _same(res, both, f"degree {degree} accumulated", SPL)


def test_certified_splines_special_rows(fresh_world, torch_cuda):
    """c1 (robot items only), thr 0.01, bad knots, a non-finite control point, a non-finite grasp."""
    from spline_continuous_ref import reference_spline_continuous
    x = _x("c1")
    ctrl, knots = tc.splines(x, 3)
    ref = tc.spline_ref(x, "c1", False, 3)
    assert min(tc.shares(ref[2])) >= 3
    _same(x.dev.held_spline_continuous(x.held, ctrl, knots, 3), ref, "c1", SPL)
    hm = hc.held_model(x.sm, x.spec)
    ref = reference_spline_continuous(hm, Oracle(hm), ctrl[:20], knots, 3, threshold=0.01, max_iter=5)[:3]
    _same(x.dev.held_spline_continuous(x.held, ctrl[:20], knots, 3, threshold=0.01, max_iter=5), ref, "thr 0.01, max_iter 5", SPL)
    c2 = ctrl[:20].copy()
    c2[3, 2, 1] = np.nan
    c2[5, :] = c2[5, :1]                                 # it does not move: V = 0
    ref = reference_spline_continuous(hm, Oracle(hm), c2, knots, 3)[:3]
    assert ref[2][3] == DEGENERATE and ref[2][5] == DEGENERATE
    _same(x.dev.held_spline_continuous(x.held, c2, knots, 3), ref, "degenerate trajectories", SPL)
    uneven = knots.copy(); uneven[4] = 0.2; uneven[5] = 0.2   # a double knot: an empty span
    ref = reference_spline_continuous(hm, Oracle(hm), ctrl[:20], uneven, 3)[:3]
    assert 0 < (ref[2] == FREE).sum() < 20
    _same(x.dev.held_spline_continuous(x.held, ctrl[:20], uneven, 3), ref, "a double knot", SPL)
    for bad in (knots[::-1].copy(), np.where(np.arange(knots.size) == 4, np.nan, knots), knots + 0.1):
        valid, t_free, st = x.dev.held_spline_continuous(x.held, ctrl[:20], bad, 3)
        assert not valid.any() and np.isnan(t_free).all() and (st == DEGENERATE).all(), "bad knots"
    G = x.spec.G.copy(); G[1, 1] = np.nan
    valid, t_free, st = x.dev.held_spline_continuous(x.held, c2, knots, 3, pose=G)
    live = np.ones(20, dtype=bool); live[[3, 5]] = False
    assert not valid.any() and np.isnan(t_free).all() and (st[live] == UNDECIDED).all() and (st[~live] == DEGENERATE).all()


# ---- 4. sampled splines --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c3", "c2"))
def test_sampled_splines(fresh_world, torch_cuda, name):
    torch = torch_cuda
    from spline_ref import reference_splines
    x = _x(name)
    ctrl, knots = tc.splines(x, 3)
    ref = tc.sampled_ref(x, name)
    assert 0 < ref[0].sum() < tc.N_SPLINES
    for S in tc.SPLINE_COUNTS:
        got = x.dev.held_spline_validity(x.held, ctrl[:S], knots, 3, tc.RESOLUTION)
        _same(got, tuple(a[:S] for a in ref), f"{name} S={S}", SMP)
    # accumulated into spline_validity's result: the reference on the combined model
    both = tc.sampled_ref(x, name, True)
    ct = torch.from_numpy(ctrl).cuda()
    res = x.dev.spline_validity(ct, knots, 3, tc.RESOLUTION)
    own = res[0].cpu().numpy().astype(bool)
    assert x.dev.held_spline_validity(x.held, ct, knots, 3, tc.RESOLUTION, out=res)[0] is res[0]
    _same(res, both, f"{name} accumulated", SMP)
    if name == "c3":
        assert (own & ~both[0]).sum() >= 3, "the held box rejects trajectories the scene lets through"
        for degree, thr in ((1, 0.01), (5, 0.0)):
            c, kn = tc.splines(x, degree, S=33)
            r = reference_splines(Oracle(hc.held_model(x.sm, x.spec)), c, kn, degree, tc.RESOLUTION, thr)
            assert 0 < r[0].sum() < 33
            _same(x.dev.held_spline_validity(x.held, c, kn, degree, tc.RESOLUTION, threshold=thr), r, f"degree {degree} thr={thr}", SMP)
        # bad knots: no samples; a non-finite grasp: hit at the first sample
        valid, t_hit, ns = x.dev.held_spline_validity(x.held, ctrl, knots[::-1].copy(), 3, tc.RESOLUTION)
        assert not valid.any() and np.isnan(t_hit).all() and (ns == 0).all()
        G = x.spec.G.copy(); G[0, 0] = np.nan
        valid, t_hit, ns = x.dev.held_spline_validity(x.held, ctrl, knots, 3, tc.RESOLUTION, pose=G)
        assert not valid.any() and (t_hit == 0.0).all() and np.array_equal(ns, ref[2])


# ---- 5. connectors -------------------------------------------------------------------------------------------------------------------
def test_continuous_connector_with_a_held_object(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector, DiscreteConnector
    from numbotics_amd.planning import unit_bspline
    x = _x("c3")
    s, g = tc.edges(x)
    both = tc.edge_ref(x, "c3", True)
    p = ConnectorParams(arm=x.arm, resolution=tc.RESOLUTION, max_distance=tc.MAXD)
    con, plain = ContinuousConnector(p, attached=x.att), ContinuousConnector(p)
    got = con.certify_batch(s, g)
    assert all(isinstance(a, np.ndarray) for a in got)
    _same(got, both, "certify_batch", CERT)
    # ... which is the accumulated engine calls
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    res = x.dev.edge_continuous(st, gt, tc.MAXD)
    x.dev.held_edge_continuous(x.held, st, gt, tc.MAXD, out=(res[0], res[2], res[3]))
    dev_got = con.certify_batch(st, gt)
    for a, b in zip(dev_got, res):
        assert a.is_cuda and torch.equal(a, b)
    # an edge the scene accepts and the held box rejects
    own = plain.certify_batch(s, g)
    pick = np.flatnonzero((own[3] == FREE) & (both[3] != FREE))
    assert pick.size >= 20
    e = int(pick[0])
    assert plain.connect(s[e], g[e]) is not None and con.connect(s[e], g[e]) is None and con.steer(s[e], g[e]) is None
    f = int(np.flatnonzero(both[3] == FREE)[0])
    assert np.array_equal(con.connect(s[f], g[f]), g[f])
    assert np.array_equal(con.connect_batch(s, g), both[0]) and np.array_equal(con.steer_batch(s, g)[0], both[0])
    hit = Oracle(hc.held_model(x.sm, x.spec, keep_scene=True)).validity(x.q[:16], 0.0)
    assert 0 < hit.sum() < 16 and np.array_equal(np.array([con.is_valid(x.q[b]) for b in range(16)]), ~hit)
    # trajectories: the connector's attachment by default, on both connectors by keyword
    ctrl, knots = tc.splines(x, 3)
    _same(con.validate_trajectories(ctrl, degree=3), tc.spline_ref(x, "c3", True, 3), "certified trajectories", SPL)
    _same(plain.validate_trajectories(ctrl, degree=3, attached=x.att), tc.spline_ref(x, "c3", True, 3), "certified, by keyword", SPL)
    dcon = DiscreteConnector(ConnectorParams(arm=x.arm, attached=x.att, resolution=tc.RESOLUTION, max_distance=tc.MAXD))
    dplain = DiscreteConnector(p)
    smp = tc.sampled_ref(x, "c3", True)
    _same(dcon.validate_trajectories(ctrl, degree=3, attached=x.att), smp, "sampled trajectories", SMP)
    _same(dplain.validate_trajectories(ctrl, degree=3, attached=x.att), smp, "sampled trajectories, params without one", SMP)
    k = int(np.flatnonzero(~smp[0])[0])
    ok, t_hit = dcon.validate_trajectory(unit_bspline(ctrl[k], degree=3), attached=x.att)
    assert ok is False and t_hit == smp[1][k]
    ok, t_free = con.validate_trajectory(unit_bspline(ctrl[k], degree=3))
    assert ok is False


def test_connectors_scene_cloud_and_held(fresh_world, torch_cuda):
    """With a cloud as well: the connector's result is scene, then cloud, then held object, done by hand with the engine."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector, DiscreteConnector
    from cloud_cases import scan
    x = _x("c3")
    s, g = tc.edges(x)
    cloud = PointCloud(np.ascontiguousarray(scan(65, seed=65)), 0.02)
    base = x.sm.links[x.sm.rshape_link[0]]._name
    shapes = x.arm._cloud_shapes(x.sm, (base,))
    p = ConnectorParams(arm=x.arm, resolution=tc.RESOLUTION, max_distance=tc.MAXD)
    con = ContinuousConnector(p, cloud=cloud, cloud_ignore_links=(base,), attached=x.att)
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    res = x.dev.edge_continuous(st, gt, tc.MAXD)
    scene = [a.cpu().numpy().copy() for a in res]
    acc = (res[0], res[2], res[3])
    x.dev.cloud_edge_continuous(cloud, st, gt, tc.MAXD, look_ahead=con.look_ahead, shapes=shapes, out=acc)
    with_cloud = res[3].cpu().numpy().copy()
    x.dev.held_edge_continuous(x.held, st, gt, tc.MAXD, out=acc)
    final = res[3].cpu().numpy()
    assert ((scene[3] == FREE) & (with_cloud != FREE)).sum() >= 3 and ((with_cloud == FREE) & (final != FREE)).sum() >= 3 \
        and (final == FREE).sum() >= 3, "each of the three stops edges of its own"
    _same(con.certify_batch(s, g), tuple(a.cpu().numpy() for a in res), "scene, cloud, held: edges", CERT)
    # trajectories, certified and sampled
    ctrl, knots = tc.splines(x, 3)
    ct = torch.from_numpy(ctrl).cuda()
    r = x.dev.spline_continuous(ct, knots, 3)
    x.dev.cloud_spline_continuous(cloud, ct, knots, 3, look_ahead=con.look_ahead, shapes=shapes, out=r)
    x.dev.held_spline_continuous(x.held, ct, knots, 3, out=r)
    _same(con.validate_trajectories(ctrl, degree=3, cloud=cloud), tuple(a.cpu().numpy() for a in r), "scene, cloud, held: certified splines", SPL)
    dcon = DiscreteConnector(p)
    r = x.dev.spline_validity(ct, knots, 3, tc.RESOLUTION)
    x.dev.cloud_spline_validity(cloud, ct, knots, 3, tc.RESOLUTION, shapes=shapes, out=r)
    after_cloud = r[0].cpu().numpy().astype(bool).copy()
    x.dev.held_spline_validity(x.held, ct, knots, 3, tc.RESOLUTION, out=r)
    assert (after_cloud & ~r[0].cpu().numpy().astype(bool)).sum() >= 1
    _same(dcon.validate_trajectories(ctrl, degree=3, cloud=cloud, cloud_ignore_links=(base,), attached=x.att),
          tuple(a.cpu().numpy() for a in r), "scene, cloud, held: sampled splines", SMP)
