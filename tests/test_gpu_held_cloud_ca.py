"""Certified edges and splines of the held object against point clouds on the device (nbk_edge_held_cloud_continuous_batch,
nbk_spline_held_cloud_continuous_batch, DeviceModel.held_cloud_edge_continuous / held_cloud_spline_continuous,
ContinuousConnector(attached_sees_cloud=True)): everything bit-equal to the NumPy + CPU-oracle restatements of the cloud's certified
entries on a model that holds the held shapes as robot shapes of the holding frame, selected on those shapes
(tests/held_cloud_ca_cases.py).  Needs a real MI355X.

Every set of 100 or more trajectories asserts on the REFERENCE, before comparing, that at least 10 % are FREE, at least 10 % are
COLLISION and at most 5 % are UNDECIDED; tests/test_held_cloud_ca_host.py pins the same conditions without a GPU."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from test_gpu_parity import assert_bitwise, torch_cuda      # noqa: F401  (fixture)
from ca_ref import FREE, COLLISION, UNDECIDED
from cloud_continuous_ref import EXIT_INF, EXIT_CAP, dense_cloud_min_distance
from cloud_spline_continuous_ref import dense_cloud_spline_min_distance
import cloud_cases as cc
import held_cases as hc
import held_cloud_cases as hcc
import held_cloud_ca_cases as hca

INF = float("inf")
DEGENERATE = 3


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same4(got, ref, what):
    """(valid, end, t_free, status) against the reference, float bits included."""
    v, end, t, st = (_np(a) for a in got)
    assert np.array_equal(v.astype(bool), ref[0]), f"{what}: valid differs at {np.flatnonzero(v.astype(bool) != ref[0])[:8]}"
    assert_bitwise(end, ref[1], f"{what}: end")
    assert_bitwise(t, ref[2], f"{what}: t_free")
    assert st.dtype == np.int32 and np.array_equal(st, ref[3]), f"{what}: status differs at {np.flatnonzero(st != ref[3])[:8]}"


def _same3(got, ref, what):
    """(valid, t_free, status) against the reference, float bits included."""
    v, t, st = (_np(a) for a in got)
    assert np.array_equal(v.astype(bool), ref[0]), f"{what}: valid differs at {np.flatnonzero(v.astype(bool) != ref[0])[:8]}"
    assert_bitwise(t, ref[1], f"{what}: t_free")
    assert st.dtype == np.int32 and np.array_equal(st, ref[2]), f"{what}: status differs at {np.flatnonzero(st != ref[2])[:8]}"


def _x(name, att=None):
    x = hca.scene(name, att)
    x.dev, x.held = x.att._device(x.arm)
    return x


def _cloud(name, **kw):
    from numbotics_amd.physics import PointCloud
    pts, r = hcc.scan(name)
    return PointCloud(pts, r, **kw), pts, r


def _mixed(status, what):
    assert (status == FREE).any() and (status == COLLISION).any(), f"{what}: {hca.shares(status)} -- not a mixed case"


def _Tf(s, g, maxd, mode, dist=None):
    from continuous_ref import edge_span
    return [edge_span(s[e], g[e], None if dist is None else dist[e], maxd, mode) for e in range(s.shape[0])]


# ---- 1. certified edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", ("dense", "sparse"))
@pytest.mark.parametrize("name", ("c2", "c1"))
def test_edges(fresh_world, torch_cuda, name, scan):
    x = _x(name)
    cloud, pts, r = _cloud(scan)
    s, g = hca.edges(x)
    hm, shapes = hcc.held_robot_model(x.sm, x.spec)
    for mode, thr, la in itertools.product(("connect", "steer"), hca.THRESHOLDS, (None,) + hca.LOOK_AHEADS):
        maxd = hca.MAXD if mode == "connect" else hca.MAXD_STEER
        look = INF if la is None else la                            # (None: the default, which is inf)
        ref = hca.edge_ref(x, name, scan, mode, thr, look)
        what = f"{name} {scan} {mode} thr={thr} look_ahead={la}"
        hca.assert_shares(ref[3], what)
        assert ref[6][EXIT_INF] > 0, f"{what}: the +inf exit must be taken"
        assert (ref[6][EXIT_CAP] > 0) == (look == 0.05), f"{what}: the cap exit is taken with look_ahead = 0.05 only"
        kw = dict(mode=mode, threshold=thr, max_iter=hca.MAX_ITER) if la is None else dict(mode=mode, threshold=thr, look_ahead=la)
        for E in hca.EDGE_COUNTS:
            got = x.dev.held_cloud_edge_continuous(x.held, cloud, s[:E], g[:E], maxd, **kw)
            assert got[0].dtype == bool
            _same4(got, tuple(a[:E] for a in ref[:4]), f"{what} E={E}")
        # soundness, independent of the reference's loop: no sample of an edge called FREE is closer than thr
        if name == "c2" and la is None:
            spans = _Tf(s, g, maxd, mode)
            free = np.flatnonzero(_np(got[3]) == FREE)
            assert free.size >= 20
            for e in free:
                d = dense_cloud_min_distance(hm, pts, r, shapes, s[e], g[e], spans[e][1], n=SOUND_SAMPLES[scan])
                assert d >= thr, f"{what}: edge {e} is called FREE and comes as close as {d}"


SOUND_SAMPLES = {"dense": 60, "sparse": 400}        # samples per edge of the soundness check: about 0.0025 / 0.0004 of joint-space length apart


def test_edge_bodies(fresh_world, torch_cuda):
    """One held body of each kind on the gripper, one after the other."""
    import types
    from numbotics_amd.scenes import build_scene, sample_q
    arm, chain, obs = build_scene("c2")
    q = sample_q(chain, 2000, seed=3)
    cloud, pts, r = _cloud("dense")
    E = 65
    for kind, body in hcc.kind_bodies().items():
        att = arm.attach(body, "gripper", pose=hc.trans(0.0, 0.0, hc.BOX_Z))
        x = types.SimpleNamespace(sm=arm.scene_model(), spec=att.spec(arm), q=q)
        dev, held = att._device(arm)
        assert int(x.spec.n_shapes) == 1
        s, g = hca.edges(x, E)
        ref = hca.edge_reference(x, pts, r, s, g, hca.MAXD)
        _mixed(ref[3], kind)
        _same4(dev.held_cloud_edge_continuous(held, cloud, s, g, hca.MAXD), ref[:4], f"held {kind}")
        ref = hca.edge_reference(x, pts, r, s, g, hca.MAXD_STEER, "steer", 0.01, 0.05)
        _same4(dev.held_cloud_edge_continuous(held, cloud, s, g, hca.MAXD_STEER, mode="steer", threshold=0.01, look_ahead=0.05),
               ref[:4], f"held {kind}, steer")
    del obs


def test_edge_eight_shapes(fresh_world, torch_cuda):
    x = _x("c2", hca.eight_att)
    assert int(x.spec.n_shapes) == 8
    cloud, pts, r = _cloud("dense")
    s, g = hca.edges(x)
    ref = hca.edge_reference(x, pts, r, s, g, hca.MAXD)
    hca.assert_shares(ref[3], "H = 8")
    # at least two different held shapes stop an edge first
    stop, st = ref[4], ref[5]
    first = {int(np.argmin(np.where(st[e] == FREE, np.inf, stop[e]))) for e in np.flatnonzero(ref[3] != FREE) if ref[3][e] != DEGENERATE}
    assert len(first) >= 2, f"the held shapes that stop an edge first: {first}"
    for E in (65, 200):
        _same4(x.dev.held_cloud_edge_continuous(x.held, cloud, s[:E], g[:E], hca.MAXD), tuple(a[:E] for a in ref[:4]), f"H = 8 E={E}")
    ref = hca.edge_reference(x, pts, r, s[:65], g[:65], hca.MAXD, thr=0.01, look_ahead=0.05)
    _same4(x.dev.held_cloud_edge_continuous(x.held, cloud, s[:65], g[:65], hca.MAXD, threshold=0.01, look_ahead=0.05), ref[:4],
           "H = 8, look_ahead 0.05")


# ---- 2. special rows -----------------------------------------------------------------------------------------------------------------
def test_special_rows(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    x = _x("c2")
    cloud, pts, r = _cloud("dense")
    s, g = hca.special_edges(x)
    # a degenerate edge, connect and steer (edges cut at T_f < 1)
    for mode, maxd in (("connect", hca.MAXD), ("steer", hca.MAXD_STEER)):
        ref = hca.edge_ref(x, "c2", "dense", mode, 0.0, INF, True)
        assert ref[3][7] == DEGENERATE and not ref[0][7] and np.isnan(ref[2][7]) and np.isnan(ref[1][7]).all()
        if mode == "steer":
            cut = np.array([sp is not None and sp[1] < 1.0 for sp in _Tf(s, g, maxd, mode)])
            assert (cut & (ref[3] == FREE)).sum() >= 5 and (~cut & (ref[3] == FREE)).sum() >= 5
            assert (ref[2][cut & (ref[3] == FREE)] < 1.0).all(), "an edge cut by steer is FREE at T_f < 1"
        for E in (65, 200):
            _same4(x.dev.held_cloud_edge_continuous(x.held, cloud, s[:E], g[:E], maxd, mode=mode), tuple(a[:E] for a in ref[:4]),
                   f"special rows {mode} E={E}")
    # dist given, and with it a NaN in a start row: q(0) is not finite, the item stops UNDECIDED there
    E = 65
    sn, gn, given = hca.nan_edges(x, E)
    for mode, maxd in (("connect", hca.MAXD), ("steer", hca.MAXD_STEER)):
        ref = hca.edge_reference(x, pts, r, sn, gn, maxd, mode, 0.01, 0.05, dist=given)
        _mixed(ref[3], f"dist given, {mode}")
        assert ref[3][11] == UNDECIDED and not ref[0][11] and ref[2][11] == 0.0 and ref[3][7] == DEGENERATE
        _same4(x.dev.held_cloud_edge_continuous(x.held, cloud, sn, gn, maxd, mode=mode, threshold=0.01, look_ahead=0.05, dist=given),
               ref[:4], f"dist given, {mode}")
    s, g = s[:E], g[:E]
    base = hca.edge_reference(x, pts, r, s, g, hca.MAXD)
    live = base[3] != DEGENERATE
    held_all = (np.zeros(E, dtype=bool), base[1], np.full(E, np.nan), np.where(live, UNDECIDED, DEGENERATE).astype(np.int32))
    # an empty cloud: every non-degenerate edge is FREE at T_f
    empty = PointCloud(np.zeros((0, 3)), 0.01, bounds=([-1, -1, 0], [1, 1, 1]), capacity=8)
    ref = hca.edge_reference(x, np.zeros((0, 3)), 0.01, s, g, hca.MAXD_STEER, "steer")
    assert (ref[3][live] == FREE).all() and ref[0][live].all() and ref[3][7] == DEGENERATE
    _same4(x.dev.held_cloud_edge_continuous(x.held, empty, s, g, hca.MAXD_STEER, mode="steer"), ref[:4], "an empty cloud")
    # a cloud whose status is set (an update with a point that is not finite, which the update refuses): 0 / NaN / UNDECIDED
    other = PointCloud(pts, r)
    bad = pts.copy()
    bad[123, 1] = np.nan
    other.update(bad)
    assert other.status() == 2
    _same4(x.dev.held_cloud_edge_continuous(x.held, other, s, g, hca.MAXD), held_all, "cloud status set")
    other.update(pts)
    assert other.status() == 0
    _same4(x.dev.held_cloud_edge_continuous(x.held, other, s, g, hca.MAXD), base[:4], "after a clean update")
    # a grasp that is not finite: 0 / NaN / UNDECIDED; another grasp; the grasp as a device tensor rewritten between two calls
    rng = np.random.default_rng(4)
    Gs = [hc.rot_pose(rng) for _ in range(2)]
    nf = Gs[0].copy()
    nf[1, 3] = np.inf
    _same4(x.dev.held_cloud_edge_continuous(x.held, cloud, s, g, hca.MAXD, pose=nf), held_all, "a grasp that is not finite")
    Gt = torch.from_numpy(Gs[0].copy()).cuda()
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    seen = []
    for k in (0, 1):
        Gt.copy_(torch.from_numpy(Gs[k].copy()).cuda())
        ref = hca.edge_reference(x, pts, r, s, g, hca.MAXD, G=Gs[k])
        _mixed(ref[3], f"grasp {k}")
        got = x.dev.held_cloud_edge_continuous(x.held, cloud, st, gt, hca.MAXD, pose=Gt)
        assert got[0].is_cuda and got[0].dtype == torch.bool and got[3].dtype == torch.int32
        _same4(got, ref[:4], f"grasp tensor, value {k}")
        _same4(x.dev.held_cloud_edge_continuous(x.held, cloud, s, g, hca.MAXD, pose=Gs[k]), ref[:4], f"grasp from the host, value {k}")
        seen.append(ref[2].tobytes())
    assert seen[0] != seen[1] and seen[0] != base[2].tobytes(), "the grasps change the results"
    Gt.copy_(torch.from_numpy(nf).cuda())
    _same4(x.dev.held_cloud_edge_continuous(x.held, cloud, st, gt, hca.MAXD, pose=Gt), held_all, "grasp tensor, not finite")
    with pytest.raises(ValueError):
        x.dev.held_cloud_edge_continuous(x.held, cloud, s, g, hca.MAXD, pose=np.zeros((E, 4, 4)))


# ---- 3. accumulate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("connect", "steer"))
def test_accumulate(fresh_world, torch_cuda, mode):
    """edge_continuous, cloud_edge_continuous(out=), held_edge_continuous(out=), held_cloud_edge_continuous(out=): the reference
    reduced over all four item sets."""
    torch = torch_cuda
    x = _x("c2")
    cloud, pts, r = _cloud("sparse")
    E = 65
    s, g = hca.special_edges(x, E)
    maxd = hca.MAXD if mode == "connect" else hca.MAXD_STEER
    for thr, la in ((0.0, INF), (0.01, 0.05)):
        stops, sts, Tf, live = hca.four_step_items(x, pts, r, s, g, maxd, mode, thr, la)
        three = hca.reduce_steps(stops, sts, Tf, live, 3)
        four = hca.reduce_steps(stops, sts, Tf, live, 4)
        assert (three[2] != four[2]).sum() >= 2, "the fourth step must change edges the three steps decide otherwise"
        assert (four[2] == FREE).any() and (four[2] != FREE).any()
        st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
        kw = dict(mode=mode, threshold=thr)
        res = x.dev.edge_continuous(st, gt, maxd, **kw)
        out = (res[0], res[2], res[3])
        x.dev.cloud_edge_continuous(cloud, st, gt, maxd, look_ahead=la, shapes=x.shapes, out=out, **kw)
        x.dev.held_edge_continuous(x.held, st, gt, maxd, out=out, **kw)
        _same3(out, three, f"{mode} thr={thr}: the three steps")
        got = x.dev.held_cloud_edge_continuous(x.held, cloud, st, gt, maxd, look_ahead=la, out=out, **kw)
        assert got[0] is res[0] and got[2] is res[2] and got[3] is res[3]
        _same3(out, four, f"{mode} thr={thr}: the four steps")
        assert_bitwise(_np(got[1]), _np(res[1]), "end")
    with pytest.raises(ValueError):
        x.dev.held_cloud_edge_continuous(x.held, cloud, st, gt, maxd, out=(res[0], res[2]))


# ---- 4. certified splines ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", (1, 2, 3, 4, 5))
def test_splines(fresh_world, torch_cuda, degree):
    torch = torch_cuda
    x = _x("c2")
    ctrl, knots = hca.splines(x, degree)
    assert ctrl.shape[1] == 8
    hm, shapes = hcc.held_robot_model(x.sm, x.spec)
    for scan in ("dense", "sparse"):
        cloud, pts, r = _cloud(scan)
        for thr in hca.THRESHOLDS:
            ref = hca.spline_ref(x, "c2", scan, degree, thr)
            what = f"degree {degree} {scan} thr={thr}"
            hca.assert_shares(ref[2], what)
            for S in hca.SPLINE_COUNTS:
                got = x.dev.held_cloud_spline_continuous(x.held, cloud, ctrl[:S], knots, degree, threshold=thr)
                assert got[0].dtype == bool
                _same3(got, tuple(a[:S] for a in ref[:3]), f"{what} S={S}")
        # soundness: no sample of a trajectory called FREE is closer than the threshold
        free = np.flatnonzero(_np(got[2]) == FREE)
        assert free.size >= 10
        for i in free[:: 1 if scan == "sparse" else 4]:
            d = dense_cloud_spline_min_distance(hm, pts, r, shapes, ctrl[i], knots, degree, n=SOUND_SAMPLES[scan])
            assert d >= hca.THRESHOLDS[-1], f"degree {degree} {scan}: trajectory {i} is called FREE and comes as close as {d}"
    # look_ahead = 0.05: the cap exit
    ref = hca.spline_ref(x, "c2", "dense", degree, 0.0, 0.05)
    assert ref[5][EXIT_CAP] > 0 and ref[5][EXIT_INF] > 0
    hca.assert_shares(ref[2], f"degree {degree}, look_ahead 0.05")
    cloud, pts, r = _cloud("dense")
    _same3(x.dev.held_cloud_spline_continuous(x.held, cloud, ctrl, knots, degree, look_ahead=0.05), ref[:3], f"degree {degree}, look_ahead 0.05")
    if degree != 3:
        return
    # accumulated behind the three existing steps: the reduction over all four item sets
    S = 65
    stops, sts, live = hca.four_step_spline_items(x, pts, r, ctrl[:S], knots, 3)
    three = hca.reduce_steps(stops, sts, np.ones(S), live, 3)
    four = hca.reduce_steps(stops, sts, np.ones(S), live, 4)
    assert (three[2] != four[2]).sum() >= 1
    ct = torch.from_numpy(ctrl[:S]).cuda()
    res = x.dev.spline_continuous(ct, knots, 3)
    x.dev.cloud_spline_continuous(cloud, ct, knots, 3, shapes=x.shapes, out=res)
    x.dev.held_spline_continuous(x.held, ct, knots, 3, out=res)
    _same3(res, three, "splines: the three steps")
    got = x.dev.held_cloud_spline_continuous(x.held, cloud, ct, knots, 3, out=res)
    assert all(a is b for a, b in zip(got, res))
    _same3(res, four, "splines: the four steps")
    # another grasp; one that is not finite; a set cloud status; an empty cloud; a degenerate trajectory
    G = hc.rot_pose(np.random.default_rng(4))
    c = ctrl[:S].copy()
    c[5] = c[5, :1]                                              # every control point the same: degenerate
    ref = hca.spline_reference(x, pts, r, c, knots, 3, G=G)
    assert ref[2][5] == DEGENERATE
    _mixed(ref[2], "splines, another grasp")
    _same3(x.dev.held_cloud_spline_continuous(x.held, cloud, c, knots, 3, pose=G), ref[:3], "splines, another grasp")
    held_all = (np.zeros(S, dtype=bool), np.full(S, np.nan), np.where(ref[2] == DEGENERATE, DEGENERATE, UNDECIDED).astype(np.int32))
    nf = G.copy()
    nf[2, 2] = np.nan
    _same3(x.dev.held_cloud_spline_continuous(x.held, cloud, c, knots, 3, pose=nf), held_all, "splines, a grasp that is not finite")
    from numbotics_amd.physics import PointCloud
    other = PointCloud(pts, r)
    bad = pts.copy()
    bad[7, 0] = np.inf
    other.update(bad)
    assert other.status() == 2
    _same3(x.dev.held_cloud_spline_continuous(x.held, other, c, knots, 3), held_all, "splines, cloud status set")
    empty = PointCloud(np.zeros((0, 3)), 0.01, bounds=([-1, -1, 0], [1, 1, 1]), capacity=8)
    v, t, st = x.dev.held_cloud_spline_continuous(x.held, empty, c, knots, 3)
    keep = ref[2] != DEGENERATE
    assert v[keep].all() and (t[keep] == 1.0).all() and (st[keep] == FREE).all() and st[5] == DEGENERATE and not v[5]


def test_the_cut_uses_the_largest_span_bound(fresh_world, torch_cuda):
    """A slow first span and a fast later one that reaches a point: D_end from the current span's bound would free it."""
    from numbotics_amd.physics import PointCloud
    x = _x("c2")
    c, kn, k, pt, r = hca.fast_last_span(x)
    hm, shapes = hcc.held_robot_model(x.sm, x.spec)
    sound = hca.spline_reference(x, pt, r, c, kn, k)
    unsound = hca.spline_reference(x, pt, r, c, kn, k, per_span_cut=True)
    assert unsound[2][0] == FREE, "a per-span D_end must free this trajectory: that is what makes it a test of the cut"
    assert sound[2][0] in (COLLISION, UNDECIDED)
    assert dense_cloud_spline_min_distance(hm, pt, r, shapes, c[0], kn, k, n=2000) < 0.0, "the trajectory does hit the point"
    got = x.dev.held_cloud_spline_continuous(x.held, PointCloud(pt, r, bounds=([-1.2, -1.2, -0.2], [1.2, 1.2, 1.6]), capacity=8), c, kn, k)
    assert got[2][0] in (COLLISION, UNDECIDED) and not got[0][0], "a trajectory that sweeps into a point on its fast last span is called free"
    _same3(got, sound[:3], "fast last span")


def test_a_linear_spline_is_the_edge(fresh_world, torch_cuda):
    """n = 2, K = 1, knots [0, 0, 1, 1]: the edge entry's bits in connect mode."""
    x = _x("c2")
    s, g = hca.special_edges(x)
    ctrl = np.ascontiguousarray(np.stack((s, g), axis=1))
    knots = np.array([0.0, 0.0, 1.0, 1.0])
    for scan, thr, la in (("dense", 0.0, INF), ("sparse", 0.01, 0.05)):
        cloud, pts, r = _cloud(scan)
        edge = x.dev.held_cloud_edge_continuous(x.held, cloud, s, g, hca.MAXD, threshold=thr, look_ahead=la)
        _mixed(edge[3], f"{scan}: the edges")
        assert (edge[3] == DEGENERATE).sum() == 1
        _same3(x.dev.held_cloud_spline_continuous(x.held, cloud, ctrl, knots, 1, threshold=thr, look_ahead=la),
               (edge[0], edge[2], edge[3]), f"{scan}: a linear spline")


# ---- 5. the case this feature exists for --------------------------------------------------------------------------------------------------
def test_a_box_carried_through_a_scanned_wall(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector
    x = _x("c1")
    out = hca.wall_edge(x)
    assert out is not None
    pts, r, s, g, t_held, cross = out
    wall = PointCloud(pts, r)
    kw = dict(cloud=wall, cloud_ignore_links=(x.base,), attached=x.att, max_iter=hca.MAX_ITER)
    p = ConnectorParams(arm=x.arm, max_distance=hca.MAXD)
    blind = ContinuousConnector(p, **kw)
    seeing = ContinuousConnector(p, attached_sees_cloud=True, **kw)
    valid, end, t_free, status = blind.certify_batch(s[None], g[None])
    assert valid[0] and status[0] == FREE and t_free[0] == 1.0, "without the flag the edge through the wall is called FREE"
    assert blind.connect(s, g) is not None
    valid, end, t_free, status = seeing.certify_batch(s[None], g[None])
    assert not valid[0] and status[0] == COLLISION and t_free[0] == t_held < cross
    assert seeing.connect(s, g) is None and seeing.steer(s, g) is None


# ---- 6. the connector ------------------------------------------------------------------------------------------------------------------
def test_connector(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    from numbotics_amd.planning import unit_bspline
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector
    x = _x("c2")
    pts, r = hcc.scan("sparse")
    cloud = PointCloud(pts, r)
    E = 65
    s, g = hca.edges(x, E)
    la = 0.05
    p = ConnectorParams(arm=x.arm, max_distance=hca.MAXD_STEER)
    kw = dict(cloud=cloud, cloud_ignore_links=(x.base,), attached=x.att, look_ahead=la, max_iter=hca.MAX_ITER)
    con = ContinuousConnector(p, attached_sees_cloud=True, **kw)
    blind = ContinuousConnector(p, **kw)
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    four = {}
    for mode in ("connect", "steer"):
        stops, sts, Tf, live = hca.four_step_items(x, pts, r, s, g, hca.MAXD_STEER, mode, 0.0, la)
        three = hca.reduce_steps(stops, sts, Tf, live, 3)
        four[mode] = hca.reduce_steps(stops, sts, Tf, live, 4)
        assert (three[2] != four[mode][2]).sum() >= 2, "the flag must change edges the three steps decide otherwise"
        assert four[mode][0].any() and not four[mode][0].all()
        got = con.certify_batch(s, g, mode)
        _same3((got[0], got[2], got[3]), four[mode], f"certify_batch {mode}, with the flag")
        # without the flag: today's three-step result, from the existing entries
        res = x.dev.edge_continuous(st, gt, hca.MAXD_STEER, mode=mode, max_iter=hca.MAX_ITER)
        o = (res[0], res[2], res[3])
        x.dev.cloud_edge_continuous(cloud, st, gt, hca.MAXD_STEER, mode=mode, look_ahead=la, shapes=x.shapes, out=o)
        x.dev.held_edge_continuous(x.held, st, gt, hca.MAXD_STEER, mode=mode, out=o)
        old = blind.certify_batch(s, g, mode)
        _same3((old[0], old[2], old[3]), tuple(_np(a) if i else _np(a).astype(bool) for i, a in enumerate(o)), f"certify_batch {mode}, without")
        _same3((old[0], old[2], old[3]), three, f"certify_batch {mode}, without the flag: the three-step reference")
        assert_bitwise(got[1], _np(res[1]), "end")
    assert np.array_equal(con.connect_batch(s, g), four["connect"][0])
    ok, end = con.steer_batch(s, g)
    assert np.array_equal(ok, four["steer"][0])
    on_dev = con.connect_batch(st, gt)
    assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy().astype(bool), four["connect"][0])
    ref = four["connect"][0]
    differ = np.flatnonzero(blind.connect_batch(s, g) != ref)
    for e in np.concatenate((np.flatnonzero(ref)[:2], np.flatnonzero(~ref)[:2], differ[:2])):
        assert (con.connect(s[e], g[e]) is not None) == bool(ref[e]), f"connect, edge {e}"
        out = con.steer(s[e], g[e])
        assert (out is not None) == bool(four["steer"][0][e]), f"steer, edge {e}"
        if out is not None:
            assert_bitwise(out, end[e], "steer returns traj(T_f)")
    # is_valid
    q = x.q[:32]
    both_m = hc.held_model(x.sm, x.spec, keep_scene=True)
    hit3 = Oracle(both_m).validity(q, 0.0) | cc.cloud_mask(x.sm, pts, r, q, 0.0, shapes=x.shapes)
    hit4 = hit3 | hcc.mask(x.sm, x.spec, pts, r, q, 0.0)
    assert (hit4 & ~hit3).any()
    assert np.array_equal(np.array([con.is_valid(q[b]) for b in range(32)]), ~hit4)
    assert np.array_equal(np.array([blind.is_valid(q[b]) for b in range(32)]), ~hit3)
    # smoothed trajectories
    S = 33
    ctrl, knots = hca.splines(x, 3, S=S)
    stops, sts, live = hca.four_step_spline_items(x, pts, r, ctrl, knots, 3, look_ahead=la)
    t3 = hca.reduce_steps(stops, sts, np.ones(S), live, 3)
    t4 = hca.reduce_steps(stops, sts, np.ones(S), live, 4)
    assert (t3[2] != t4[2]).sum() >= 1 and t4[0].any() and not t4[0].all()
    _same3(con.validate_trajectories(ctrl, degree=3, cloud=cloud), t4, "validate_trajectories with the flag")
    _same3(blind.validate_trajectories(ctrl, degree=3, cloud=cloud), t3, "validate_trajectories without the flag")
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        con.validate_trajectories(ctrl, degree=3)
    for i in np.concatenate((np.flatnonzero(t4[0])[:1], np.flatnonzero(t3[2] != t4[2])[:1])):
        ok, t = con.validate_trajectory(unit_bspline(ctrl[i], 3), cloud=cloud)
        assert ok == bool(t4[0][i]) and (t == t4[1][i] or (np.isnan(t) and np.isnan(t4[1][i]))), f"validate_trajectory {i}"


# ---- 7. capture ----------------------------------------------------------------------------------------------------------------------
def test_capture(fresh_world, torch_cuda):
    """The four edge steps in one captured graph, a linear chain; replays follow the cloud's update and the grasp tensor rewritten in
    place, and equal a direct call on the same inputs.  A call that allocated or synchronised inside the capture would end it with an
    error."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    x = _x("c2")
    E = 65
    s, g = hca.edges(x, E)
    rng = np.random.default_rng(9)
    Gs = [hc.rot_pose(rng) for _ in range(3)]
    clouds = [np.ascontiguousarray(cc.scan(1000, seed=k)) for k in range(3)]
    r = 0.01
    cloud = PointCloud(clouds[0], r, bounds=([-0.6, -0.6, 0.0], [0.6, 0.6, 1.0]))
    Gt = torch.from_numpy(Gs[0].copy()).cuda()
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()

    def chain():
        res = x.dev.edge_continuous(st, gt, hca.MAXD)
        out = (res[0], res[2], res[3])
        x.dev.cloud_edge_continuous(cloud, st, gt, hca.MAXD, shapes=x.shapes, out=out)
        x.dev.held_edge_continuous(x.held, st, gt, hca.MAXD, pose=Gt, out=out)
        x.dev.held_cloud_edge_continuous(x.held, cloud, st, gt, hca.MAXD, pose=Gt, out=out)
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                  # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = chain()
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for k in (1, 2):
        cloud.update(clouds[k])
        Gt.copy_(torch.from_numpy(Gs[k].copy()).cuda())
        graph.replay()
        torch.cuda.synchronize()
        replayed = tuple(_np(a).copy() for a in out)
        direct = tuple(_np(a) for a in chain())
        torch.cuda.synchronize()
        _same3((replayed[0], replayed[1], replayed[2]), (direct[0].astype(bool), direct[1], direct[2]), f"replay {k}: a direct call")
        stops, sts, Tf, live = hca.four_step_items(x, clouds[k], r, s, g, hca.MAXD, G=Gs[k])
        four = hca.reduce_steps(stops, sts, Tf, live, 4)
        three = hca.reduce_steps(stops, sts, Tf, live, 3)
        assert (three[2] != four[2]).any(), f"replay {k}: the new step decides edges"
        _same3(replayed, four, f"replay {k}: the four-step reference")
        seen.append(four[1].tobytes() + four[2].tobytes())
    assert seen[0] != seen[1]
