"""A mesh in the hand, on the device: held convex hulls (nbk_held_create_hulls, ``Arm.attach(..., meshes=True)``) through every
scene-side held entry -- verdicts, sampled edges and splines, distances, records, certified edges and splines, the public path --
each result bit for bit what the CPU oracle (and the NumPy restatements of the certified loops) give on the combined descriptor:
the scene's model with the held shapes as robot shapes of the holding frame and the held hulls appended to its hull tables
(tests/held_hull_cases.py ``held_model_hulls``).  The held-versus-cloud entries refuse such an object.  Needs a real MI355X.

What the fixtures are relied on for -- the share of rows that collide, rows the held object decides, no sphere-versus-held-hull
item at tc <= 0 -- is pinned without a GPU by tests/test_held_hull_host.py; every mixed case asserts on the REFERENCE,
before comparing, that it has both verdicts."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from test_gpu_parity import assert_bitwise, torch_cuda      # noqa: F401  (fixture)
from ca_ref import FREE, COLLISION
import held_cases as hc
import held_hull_cases as hh
import held_records_cases as rc
import held_traj_cases as tc

NT = 8
MAXD = tc.MAXD
RES = tc.RESOLUTION
CERT = ("valid", "end", "t_free", "status")
SPL = ("valid", "t_free", "status")
SMP = ("valid", "t_hit", "n_samples")


def _mixed(mask, what):
    assert 0 < int(np.sum(mask)) < len(mask), f"{what}: {int(np.sum(mask))} of {len(mask)} -- not a mixed case"


def _x(name, kind, margins=True):
    x = hh.scene(name, kind, margins)
    x.dev = x.arm._scene_device()[1]
    x.held = x.att._device(x.arm)[1] if x.att is not None else hh.device_held(x.dev, x.spec)
    return x


def _same(got, ref, what, names):
    for a, r, n in zip(got, ref, names):
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        if r.dtype == bool:
            a = a.astype(bool)
        tc.assert_bits(a, r, f"{what}: {n}")


def _grasps(x, n, seed):
    rng = np.random.default_rng(seed)
    return [x.spec.G @ hc.rot_pose(rng, 0.3, 0.02) @ hc.trans(0, 0, -hc.BOX_Z) for _ in range(n)]


# ---- 1. verdicts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,margins", (("c2", "rock", True), ("c2", "rock", False), ("c2", "mixed", True), ("c2", "wedge", False),
                                               ("c5m", "wedge", True), ("c5m", "mixed", True), ("c5m", "mixed", False),
                                               ("c5m", "rock", False)))
def test_held_hull_verdicts(fresh_world, torch_cuda, name, kind, margins):
    """c2: primitive links and a cube; c5m: mesh links, world hulls and a plane (hull against hull, hull against plane)."""
    torch = torch_cuda
    x = _x(name, kind, margins)
    q = x.q[:1000]
    qt = torch.from_numpy(q).cuda()
    if name == "c5m":
        kinds = {int(x.sm.wshape_type[w]) for w in x.spec.world_shapes}
        assert 5 in kinds and 4 in kinds and 5 in {int(t) for t in x.sm.rshape_type[x.spec.robot_shapes]}
    for thr in hh.THRESHOLDS:
        ref = hh.held_mask(x.sm, x.spec, q, thr)
        both = Oracle(hh.held_model_hulls(x.sm, x.spec, keep_scene=True)).validity(q, thr, nthreads=NT)
        own = Oracle(x.sm).validity(q, thr, nthreads=NT)
        assert (both & ~own).sum() >= 5, "the held object must decide rows the scene lets through"
        for B in hh.BATCHES:
            what = f"{name} {kind} {'bullet' if margins else 'sharp'} thr={thr} B={B}"
            if B >= 63:
                _mixed(ref[:B], what)
            got = x.dev.held_validity(x.held, q[:B], thr)
            assert got.dtype == bool and np.array_equal(got, ref[:B]), f"{what}: bytes differ at {np.flatnonzero(got != ref[:B])[:8]}"
            words = x.dev.held_validity(x.held, q[:B], thr, packed=True)
            assert np.array_equal(words, hc.pack_bits(ref[:B])), f"{what}: packed words"
            mask = x.dev.validity(qt[:B], thr)
            assert x.dev.held_validity(x.held, qt[:B], thr, out=mask) is mask
            assert np.array_equal(mask.cpu().numpy(), both[:B]), f"{what}: accumulated bytes"
            w = x.dev.validity(qt[:B], thr, packed=True)
            x.dev.held_validity(x.held, qt[:B], thr, packed=True, out=w)
            assert np.array_equal(w.cpu().numpy(), hc.pack_bits(both[:B])), f"{what}: accumulated words"


@pytest.mark.parametrize("name,kind", (("c2", "rock"), ("c5m", "mixed")))
def test_held_hull_grasp_per_row(fresh_world, torch_cuda, name, kind):
    x = _x(name, kind)
    B = 65
    q = x.q[:B]
    G = np.array(_grasps(x, B, 65))
    ref = np.array([hh.held_mask(x.sm, x.spec, q[b], 0.0, G=G[b])[0] for b in range(B)])
    _mixed(ref, "65 grasps")
    assert (ref != hh.held_mask(x.sm, x.spec, q, 0.0)).any(), "the grasps change verdicts"
    got = x.dev.held_validity(x.held, q, 0.0, pose=G)
    assert np.array_equal(got, ref), f"a grasp per row: differs at {np.flatnonzero(got != ref)[:8]}"
    # a grasp row and a q row that are not finite collide
    free = np.flatnonzero(~ref)
    bad, qb = G.copy(), q.copy()
    bad[free[0], 1, 2] = np.nan
    qb[free[1], 3] = np.inf
    want = ref.copy(); want[free[:2]] = True
    assert np.array_equal(x.dev.held_validity(x.held, qb, 0.0, pose=bad), want)


# ---- 2. sampled edges and splines --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", (("c2", "rock"), ("c5m", "mixed")))
def test_held_hull_sampled_edges_and_splines(fresh_world, torch_cuda, name, kind):
    torch = torch_cuda
    from spline_ref import reference_splines
    x = _x(name, kind)
    hm, hb = hh.held_model_hulls(x.sm, x.spec), hh.held_model_hulls(x.sm, x.spec, keep_scene=True)
    s, g = hc.edge_set(x.q, 200)
    g[7] = s[7]                                                  # a degenerate edge
    for mode, maxd, thr in (("connect", MAXD, 0.0), ("steer", 0.4, 0.01)):
        ref = Oracle(hm).edge_validity(s, g, RES, maxd, mode=mode, threshold=thr, nthreads=NT)
        assert not ref[0][7] and ref[2][7] == 0
        _mixed(ref[0], f"edges {mode}")
        for E in (1, 64, 65, 200):
            valid, end, ns = x.dev.held_edge_validity(x.held, s[:E], g[:E], RES, maxd, mode=mode, threshold=thr)
            assert valid.dtype == bool and np.array_equal(valid, ref[0][:E]), f"{mode} E={E}: valid differs at {np.flatnonzero(valid != ref[0][:E])[:8]}"
            assert_bitwise(end, ref[1][:E], f"{mode} E={E}: end")
            assert ns.dtype == np.int32 and np.array_equal(ns, ref[2][:E]), f"{mode} E={E}: n_samples"
        both = Oracle(hb).edge_validity(s, g, RES, maxd, mode=mode, threshold=thr, nthreads=NT)
        st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
        res = x.dev.edge_validity(st, gt, RES, maxd, mode=mode, threshold=thr)
        assert (res[0].cpu().numpy().astype(bool) & ~both[0]).sum() >= 3, "the held object must block edges the scene lets through"
        out = x.dev.held_edge_validity(x.held, st, gt, RES, maxd, mode=mode, threshold=thr, out=res[0])
        assert out[0] is res[0] and np.array_equal(res[0].cpu().numpy().astype(bool), both[0]), f"{mode}: accumulated"
    ctrl, knots = tc.splines(x, 3, S=200)
    ref = reference_splines(Oracle(hm), ctrl, knots, 3, RES, 0.0)
    _mixed(ref[0], "splines")
    for S in (1, 64, 65, 200):
        _same(x.dev.held_spline_validity(x.held, ctrl[:S], knots, 3, RES), tuple(a[:S] for a in ref), f"splines S={S}", SMP)
    both = reference_splines(Oracle(hb), ctrl, knots, 3, RES, 0.0)
    ct = torch.from_numpy(ctrl).cuda()
    res = x.dev.spline_validity(ct, knots, 3, RES)
    assert x.dev.held_spline_validity(x.held, ct, knots, 3, RES, out=res)[0] is res[0]
    _same(res, both, "splines accumulated", SMP)


# ---- 3. distances and records ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", (("c2", "rock"), ("c5m", "mixed")))
def test_held_hull_distances_and_records(fresh_world, torch_cuda, name, kind):
    """Every field against the scene entries' reference on the combined descriptor: pair k of that descriptor is item k."""
    x = _x(name, kind)
    cols = tc.item_columns(x.sm, x.spec)
    K = len(cols)
    assert x.held.n_items == K and np.array_equal(x.held.items(), cols)
    q = x.q[:65]
    orc = Oracle(hh.held_model_hulls(x.sm, x.spec))
    ref = orc.proximity_jacobian(q)
    tc.assert_bits(ref[0], orc.pair_distances(q), "the reference's two distances")
    hull = np.array([x.spec.shape_type[c[0]] == hh.SH_HULL for c in cols])
    assert (ref[0][:, hull] < 0.0).any() and (ref[0][:, hull] > 0.0).any(), "a held hull that penetrates (the EPA pass) and one that does not"
    assert np.abs(ref[2]).max() > 0.1
    Gs = _grasps(x, 4, 21)
    pick = np.arange(65) % 4
    refs = [Oracle(hh.held_model_hulls(x.sm, x.spec, G)).proximity_jacobian(q) for G in Gs]
    rows_ref = rc.per_row(refs, pick)
    poses = np.stack([Gs[k] for k in pick])
    for B in (1, 65):                                     # 1: every lane another item; 65: a wave straddles two items
        tc.assert_bits(x.dev.held_distances(x.held, q[:B]), ref[0][:B], f"{name} distances B={B}")
        tc.assert_bits(x.dev.held_distances(x.held, q[:B], pose=poses[:B]), rows_ref[0][:B], f"{name} distances B={B}, a grasp per row")
        rc.assert_records(x.dev.held_records(x.held, q[:B]), ref, f"{name} records B={B}", B)
        rc.assert_records(x.dev.held_records(x.held, q[:B], pose=poses[:B]), rows_ref, f"{name} records B={B}, a grasp per row", B)
    # listed records: every (row, item) once in a shuffled order (waves of mixed items: per-lane loads) and item-major (waves of one
    # item: the hull's vertices through the scalar cache) -- the same bits; an entry out of range is NaN in every field
    dense = x.dev.held_records(x.held, q)
    bb, kk = np.meshgrid(np.arange(65), np.arange(K), indexing="ij")
    major = np.stack((bb.T.reshape(-1), kk.T.reshape(-1)), axis=1).astype(np.int32)          # item-major: 65 rows of one item in a row
    rng = np.random.default_rng(12)
    shuffled = major[rng.permutation(major.shape[0])]
    for items, what in ((major, "item-major"), (shuffled, "shuffled")):
        got = x.dev.held_records(x.held, q, items=items)
        rc.assert_records(got, [a[items[:, 0], items[:, 1]] for a in ref], f"{name} listed, {what}")
        rc.assert_records(got, [a[items[:, 0], items[:, 1]] for a in dense], f"{name} listed against dense, {what}")
    out = np.array([[-1, 0], [65, 0], [0, K], [3, -1]], dtype=np.int32)
    items = np.concatenate((shuffled[:100], out, shuffled[100:130]))
    got = x.dev.held_records(x.held, q, items=items)
    assert rc.all_nan(got, np.arange(100, 104)), "entries outside [0, B) x [0, K) are NaN in every field"
    inside = np.ones(len(items), dtype=bool); inside[100:104] = False
    rc.assert_records([a[inside] for a in got], [a[items[inside, 0], items[inside, 1]] for a in ref], f"{name} listed, beside the entries out of range")
    # the closest record
    d, it, w, j = x.dev.held_closest_records(x.held, q)
    item = ref[0].argmin(axis=1)
    b = np.arange(65)
    assert it.dtype == np.int32 and np.array_equal(it, item)
    rc.assert_records((d, w, j), (ref[0][b, item], ref[1][b, item], ref[2][b, item]), f"{name} closest records")
    assert hull[item].any(), "a held hull is the closest item somewhere"
    # rows that are not finite: NaN in every field of that row only
    qb = q.copy(); qb[3, 2] = np.nan
    got = x.dev.held_records(x.held, qb)
    assert rc.all_nan(got, [3])
    keep = b != 3
    rc.assert_records([a[keep] for a in got], [r[keep] for r in ref], f"{name}: the rows beside a NaN row")
    assert np.isnan(x.dev.held_distances(x.held, qb)[3]).all()
    pb = poses.copy(); pb[5, 1, 3] = np.nan
    assert np.isnan(x.dev.held_distances(x.held, q, pose=pb)[5]).all() and rc.all_nan(x.dev.held_records(x.held, q, pose=pb), [5])


# ---- 4. certified edges and splines ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", (("c2", "rock"), ("c5m", "mixed")))
def test_held_hull_certified(fresh_world, torch_cuda, name, kind):
    torch = torch_cuda
    from continuous_ref import reference_continuous
    from spline_continuous_ref import reference_spline_continuous
    x = _x(name, kind)
    hm, hb = hh.held_model_hulls(x.sm, x.spec), hh.held_model_hulls(x.sm, x.spec, keep_scene=True)
    s, g = hc.edge_set(x.q, 65)
    ref = reference_continuous(hm, Oracle(hm), s, g, MAXD)[:4]
    free, col, und = tc.shares(ref[3])
    assert free >= 3 and col >= 3, (free, col, und)
    for E in (1, 65):
        _same(x.dev.held_edge_continuous(x.held, s[:E], g[:E], MAXD), tuple(a[:E] for a in ref), f"{name} edges E={E}", CERT)
    both = reference_continuous(hb, Oracle(hb), s, g, MAXD)[:4]
    assert ((both[3] != FREE) & (ref[3] != FREE)).sum() >= 3
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    res = x.dev.edge_continuous(st, gt, MAXD)
    out = x.dev.held_edge_continuous(x.held, st, gt, MAXD, out=(res[0], res[2], res[3]))
    assert out[0] is res[0] and out[2] is res[2] and out[3] is res[3]
    _same((res[0], out[1], res[2], res[3]), both, f"{name} edges accumulated", CERT)
    # an edge a sampled check at its resolution accepts and the certified one rejects: looked for at three resolutions in both
    # fixtures by the references alone -- NONE WAS FOUND (every edge the certified check calls COLLISION has a colliding sample
    # already at resolution 0.5); where a later change of the fixtures gives one, the device must agree with both references on it
    for res_ in (RES, 0.2, 0.5):
        sampled = Oracle(hm).edge_validity(s, g, res_, MAXD, nthreads=NT)[0]
        for e in np.flatnonzero(sampled & (ref[3] == COLLISION))[:2]:
            assert x.dev.held_edge_validity(x.held, s[e:e + 1], g[e:e + 1], res_, MAXD)[0][0]
            assert not x.dev.held_edge_continuous(x.held, s[e:e + 1], g[e:e + 1], MAXD)[0][0]
    ctrl, knots = tc.splines(x, 3, S=65)
    ref = reference_spline_continuous(hm, Oracle(hm), ctrl, knots, 3)[:3]
    free, col, und = tc.shares(ref[2])
    assert free >= 3 and col >= 3, (free, col, und)
    for S in (1, 65):
        _same(x.dev.held_spline_continuous(x.held, ctrl[:S], knots, 3), tuple(a[:S] for a in ref), f"{name} splines S={S}", SPL)
    both = reference_spline_continuous(hb, Oracle(hb), ctrl, knots, 3)[:3]
    ct = torch.from_numpy(ctrl).cuda()
    res = x.dev.spline_continuous(ct, knots, 3)
    assert x.dev.held_spline_continuous(x.held, ct, knots, 3, out=res)[0] is res[0]
    _same(res, both, f"{name} splines accumulated", SPL)


# ---- 5. degenerate and boundary cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c2", "c5m"))
@pytest.mark.parametrize("kind", ("tetra", "flat"))
def test_held_hull_degenerate(fresh_world, torch_cuda, name, kind):
    """A 4-vertex tetrahedron and a flat hull without planes, given directly through HeldSpec."""
    x = _x(name, kind)
    assert x.spec.hull_verts.shape[0] == (4 if kind == "tetra" else 5) and (x.spec.hull_planes.shape[0] == 0) == (kind == "flat")
    q = x.q[:256]
    for thr in hh.THRESHOLDS:
        ref = hh.held_mask(x.sm, x.spec, q, thr)
        _mixed(ref, f"{name} {kind} thr={thr}")
        got = x.dev.held_validity(x.held, q, thr)
        assert np.array_equal(got, ref), f"{name} {kind} thr={thr}: differs at {np.flatnonzero(got != ref)[:8]}"
    ref = Oracle(hh.held_model_hulls(x.sm, x.spec)).pair_distances(q[:65])
    assert (ref < 0.0).any() and (ref > 0.0).any()
    for B in (1, 65):
        tc.assert_bits(x.dev.held_distances(x.held, q[:B]), ref[:B], f"{name} {kind} distances B={B}")


def test_held_hull_eight_hulls(fresh_world, torch_cuda):
    """H = 8, all hulls: eight hulls of their own in the held object's tables, each deciding somewhere."""
    from numbotics_amd.scenes import build_scene, sample_q
    arm, chain, obs = build_scene("c2")
    rng = np.random.default_rng(8)
    extra = []
    for k in range(7):
        T = hc.rot_pose(rng, 1.0, 0.0)
        T[:3, 3] = rng.uniform(-0.2, 0.2, 3)
        extra.append((hh.SH_HULL, T, (0.4 + 0.1 * (k % 3)) * (hh.TETRA if k % 2 else hh.FLAT + rng.uniform(-0.05, 0.05, hh.FLAT.shape))))
    spec, probe = hh.hull_spec(arm, 0.5 * hh.TETRA, hc.trans(0.0, 0.0, 0.3), extra=tuple(extra))
    assert spec.n_shapes == 8 and spec.n_hulls == 8 and (spec.shape_type == hh.SH_HULL).all()
    assert sorted(int(p[0]) for p in spec.shape_param) == list(range(8))
    sm = arm.scene_model()
    dev = arm._scene_device()[1]
    held = hh.device_held(dev, spec)
    q = sample_q(chain, 256, seed=3)
    for thr in hh.THRESHOLDS:
        ref = hh.held_mask(sm, spec, q, thr)
        _mixed(ref, f"H=8 thr={thr}")
        got = dev.held_validity(held, q, thr)
        assert np.array_equal(got, ref), f"H=8 thr={thr}: differs at {np.flatnonzero(got != ref)[:8]}"
    for h in range(8):
        one = dataclasses.replace(spec, shape_local=spec.shape_local[h:h + 1], shape_type=spec.shape_type[h:h + 1],
                                  shape_param=spec.shape_param[h:h + 1])
        assert hh.held_mask(sm, one, q, 0.0).any(), f"held hull {h} never collides: the fixture does not exercise it"
    tc.assert_bits(dev.held_distances(held, q[:65]), Oracle(hh.held_model_hulls(sm, spec)).pair_distances(q[:65]), "H=8 distances")
    # a ninth hull is refused
    nine = dataclasses.replace(spec, shape_local=np.concatenate((spec.shape_local, spec.shape_local[:1])),
                               shape_type=np.append(spec.shape_type, 5).astype(np.int32),
                               shape_param=np.concatenate((spec.shape_param, spec.shape_param[:1])))
    from numbotics_amd import _lib
    with pytest.raises(_lib.NbkError, match="UNSUPPORTED"):
        hh.device_held(dev, nine)
    del probe, obs


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
class _Untouched:
    """A stand-in for a PointCloud that fails the test when anything is asked of it."""

    def __getattr__(self, name):
        raise AssertionError(f"the cloud was touched: .{name}")


def test_held_hull_refusals(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd import _lib
    from numbotics_amd.engine import DeviceHeld, held_edge_shape_motion_bounds, held_spline_shape_motion_bounds
    from numbotics_amd.physics import PointCloud
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector
    from cloud_cases import scan
    x = _x("c2", "rock")
    q = x.q[:65]
    s, g = hc.edge_set(x.q, 65)
    ctrl, knots = tc.splines(x, 3, S=8)
    ghost = _Untouched()
    msg = "held meshes do not see scans yet"
    # the engine's seven calls and the Python layers on top of them
    calls = (lambda: x.dev.held_cloud_validity(x.held, ghost, q), lambda: x.dev.held_cloud_clearance(x.held, ghost, q, 0.1),
             lambda: x.dev.held_cloud_records(x.held, ghost, q, 0.1),
             lambda: x.dev.held_cloud_edge_validity(x.held, ghost, s, g, RES, MAXD),
             lambda: x.dev.held_cloud_spline_validity(x.held, ghost, ctrl, knots, 3, RES),
             lambda: x.dev.held_cloud_edge_continuous(x.held, ghost, s, g, MAXD),
             lambda: x.dev.held_cloud_spline_continuous(x.held, ghost, ctrl, knots, 3),
             lambda: x.arm.in_collision_with_attached(q, x.att, cloud=ghost),
             lambda: x.arm.attached_cloud_clearance(q, x.att, ghost, 0.1),
             lambda: x.arm.attached_cloud_proximity_jacobians(q, x.att, ghost, 0.1),
             lambda: x.arm.attached_cloud_closest_to(q[0], x.att, ghost, 0.1),
             lambda: ConnectorParams(arm=x.arm, cloud=ghost, attached=x.att, attached_sees_cloud=True),
             lambda: ContinuousConnector(ConnectorParams(arm=x.arm), cloud=ghost, attached=x.att, attached_sees_cloud=True))
    for k, f in enumerate(calls):
        with pytest.raises(ValueError, match=msg):
            f()
    # the two shape-bound host twins have no hull tables: a hull is unsupported, as for nbk_held_create
    for f in (lambda: held_edge_shape_motion_bounds(x.sm, x.spec, s, g), lambda: held_spline_shape_motion_bounds(x.sm, x.spec, ctrl, knots, 3)):
        with pytest.raises(_lib.NbkError, match="UNSUPPORTED"):
            f()
    # at the C boundary: NBK_ERR_UNSUPPORTED from all seven, and a real cloud keeps its state
    lib = _lib.load()
    pts = np.ascontiguousarray(scan(65, seed=65))
    cloud = PointCloud(pts, 0.02)
    before = cloud.status()
    qt, st, gt = torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    ct, kt = torch.from_numpy(ctrl).cuda(), torch.from_numpy(knots).cuda()
    m = torch.full((65,), 7, dtype=torch.uint8, device="cuda")
    d = torch.full((65,), 7.0, dtype=torch.float64, device="cuda")
    i32 = torch.full((65,), 7, dtype=torch.int32, device="cuda")
    ws = torch.zeros((max(x.dev.held_cloud_edge_workspace_bytes(65), x.dev.held_cloud_spline_workspace_bytes(8)),), dtype=torch.uint8, device="cuda")
    M, H, Cl = x.dev._h, x.held._h, cloud._h
    U = -4
    assert lib.nbk_held_cloud_validity_batch(M, H, Cl, qt.data_ptr(), 65, None, 0, 0.0, 0, None, m.data_ptr(), None) == U
    assert lib.nbk_held_cloud_clearance_batch(M, H, Cl, qt.data_ptr(), 65, None, 0, 0.1, d.data_ptr(), None, None, None) == U
    assert lib.nbk_held_cloud_records_batch(M, H, Cl, qt.data_ptr(), 65, None, 0, 0.1, 0, d.data_ptr(), None, None, None, None, None) == U
    assert lib.nbk_edge_held_cloud_validity_batch(M, H, Cl, st.data_ptr(), gt.data_ptr(), None, 65, RES, MAXD, 0, 0.0, None, 0, m.data_ptr(),
                                                  None, None, ws.data_ptr(), ws.numel(), None) == U
    assert lib.nbk_spline_held_cloud_validity_batch(M, H, Cl, ct.data_ptr(), 8, 6, 3, kt.data_ptr(), RES, 0.0, None, 0, m.data_ptr(), None,
                                                    None, ws.data_ptr(), ws.numel(), None) == U
    assert lib.nbk_edge_held_cloud_continuous_batch(M, H, Cl, st.data_ptr(), gt.data_ptr(), None, 65, MAXD, 0, 0.0, 64, 1e-6, 0.25, None, 0,
                                                    m.data_ptr(), None, d.data_ptr(), i32.data_ptr(), None) == U
    assert lib.nbk_spline_held_cloud_continuous_batch(M, H, Cl, ct.data_ptr(), 8, 6, 3, kt.data_ptr(), 0.0, 64, 1e-6, 0.25, None, 0,
                                                      m.data_ptr(), d.data_ptr(), i32.data_ptr(), None) == U
    torch.cuda.synchronize()
    assert (m == 7).all() and (d == 7.0).all() and (i32 == 7).all(), "a refused call writes nothing"
    assert cloud.status() == before
    # a primitive attachment is served as before
    box, b = hc.gripper_box(x.arm)
    dev2, held2 = box._device(x.arm)
    assert not held2.has_hull and dev2.held_cloud_validity(held2, cloud, q).shape == (65,)
    # without hulls= the creator still refuses type 5
    with pytest.raises(_lib.NbkError, match="UNSUPPORTED"):
        DeviceHeld(x.dev, x.spec.frame, x.spec.A, x.spec.G, x.spec.shape_type, x.spec.shape_local, x.spec.shape_param,
                   x.spec.world_shapes, x.spec.robot_shapes)
    # bad tables are answered by the creator as by the host twins
    cut = x.spec.hull_planes.copy(); cut[0, 3] -= 0.05
    with pytest.raises(_lib.NbkError, match="INVALID"):
        hh.device_held(x.dev, dataclasses.replace(x.spec, hull_planes=cut))


# ---- 7. capture --------------------------------------------------------------------------------------------------------------------
def test_held_hull_capture(fresh_world, torch_cuda):
    """One graph holding held_validity and held_distances with a hull attachment, re-grasped by rewriting the grasp tensor."""
    torch = torch_cuda
    x = _x("c2", "rock")
    B = 256
    q = x.q[:B]
    Gs = _grasps(x, 2, 9)
    qt = torch.from_numpy(q.copy()).cuda()
    Gt = torch.from_numpy(Gs[0].copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x.dev.held_validity(x.held, qt, 0.0, pose=Gt)                   # warm-up outside the capture
        x.dev.held_distances(x.held, qt, pose=Gt)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mask = x.dev.held_validity(x.held, qt, 0.0, pose=Gt)
            dist = x.dev.held_distances(x.held, qt, pose=Gt)
    torch.cuda.current_stream().wait_stream(side)
    Gt.copy_(torch.from_numpy(Gs[1].copy()).cuda())
    graph.replay()
    torch.cuda.synchronize()
    got_m, got_d = mask.cpu().numpy().astype(bool), dist.cpu().numpy()
    hm = hh.held_model_hulls(x.sm, x.spec, Gs[1])
    ref = Oracle(hm).validity(q, 0.0, nthreads=NT)
    _mixed(ref, "the replay")
    assert (ref != hh.held_mask(x.sm, x.spec, q, 0.0, G=Gs[0])).any(), "the new grasp changes verdicts"
    assert np.array_equal(got_m, x.dev.held_validity(x.held, q, 0.0, pose=Gs[1])) and np.array_equal(got_m, ref)
    tc.assert_bits(got_d, x.dev.held_distances(x.held, q, pose=Gs[1]), "replayed distances against the direct call")
    tc.assert_bits(got_d, Oracle(hm).pair_distances(q), "replayed distances against the oracle")


# ---- 8. the public path ------------------------------------------------------------------------------------------------------------
def test_held_mesh_public_path(fresh_world, torch_cuda):
    from numbotics_amd.physics import Proximity
    from numbotics_amd.planning import safe_sets
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector, DiscreteConnector
    from continuous_ref import reference_continuous
    x = _x("c5m", "rock")
    q = x.q[:130]
    hm, hb = hh.held_model_hulls(x.sm, x.spec), hh.held_model_hulls(x.sm, x.spec, keep_scene=True)
    ref = hh.held_mask(x.sm, x.spec, q, 0.0)
    _mixed(ref, "public path")
    hit = x.arm.in_collision_with_attached(q.reshape(10, 13, -1), x.att)
    assert hit.shape == (10, 13) and np.array_equal(hit.reshape(-1), ref)
    assert x.arm.in_collision_with_attached(q[0], x.att, 0.01) is bool(hh.held_mask(x.sm, x.spec, q[0], 0.01)[0])
    rec = Oracle(hm).proximity_jacobian(q)
    dist, item = x.arm.attached_clearance(q, x.att)
    tc.assert_bits(dist, rec[0].min(axis=1), "attached_clearance")
    assert np.array_equal(item, rec[0].argmin(axis=1))
    b = np.arange(130)
    want = (rec[0][b, item], rec[1][b, item], rec[2][b, item])
    d, it, w, j = x.arm.attached_proximity_jacobians(q, x.att)
    assert np.array_equal(it, item)
    rc.assert_records((d, w, j), want, "attached_proximity_jacobians")
    dg, jg = safe_sets.attached_distance_and_gradient(x.arm, q, x.att)
    rc.assert_records((dg, want[1], jg), want, "attached_distance_and_gradient")
    cols = x.held.items()
    for kind in (0, 1):
        rows = np.flatnonzero(cols[item, 1] == kind)
        assert rows.size, f"no row whose closest item is of kind {kind}"
        r = int(rows[0])
        prox = x.arm.attached_closest_to(q[r], x.att)
        assert isinstance(prox, Proximity) and (prox.target if kind == 0 else prox.subject) is x.att.objects[0]
        tc.assert_bits(np.concatenate((prox.position_on_subject, prox.position_on_target, prox.normal_target_to_subject)), want[1][r], "Proximity")
        tc.assert_bits(np.float64(prox.distance), dist[r], "Proximity.distance")
    # the connectors, on a handful of edges
    s, g = hc.edge_set(x.q, 24)
    p = ConnectorParams(arm=x.arm, attached=x.att, resolution=RES, max_distance=MAXD)
    dcon = DiscreteConnector(p)
    sampled = Oracle(hb).edge_validity(s, g, RES, MAXD, mode="connect", nthreads=NT)
    _mixed(sampled[0], "connector edges")
    assert np.array_equal(dcon.connect_batch(s, g), sampled[0])
    ccon = ContinuousConnector(ConnectorParams(arm=x.arm, resolution=RES, max_distance=MAXD), attached=x.att)
    cert = reference_continuous(hb, Oracle(hb), s, g, MAXD)[:4]
    _same(ccon.certify_batch(s, g), cert, "certify_batch", CERT)
    for e in np.concatenate((np.flatnonzero(sampled[0])[:2], np.flatnonzero(~sampled[0])[:2])):
        assert (dcon.connect(s[e], g[e]) is not None) == bool(sampled[0][e]), f"DiscreteConnector.connect, edge {e}"
    for e in np.concatenate((np.flatnonzero(cert[0])[:2], np.flatnonzero(~cert[0])[:2])):
        assert (ccon.connect(s[e], g[e]) is not None) == bool(cert[0][e]), f"ContinuousConnector.connect, edge {e}"
