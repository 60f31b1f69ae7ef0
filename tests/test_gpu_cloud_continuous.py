"""Certified continuous edges against a point cloud on the device (nbk_edge_cloud_continuous_batch, DeviceModel.cloud_edge_continuous,
ContinuousConnector(cloud=...)): valid / end / t_free / status bit-identical to the NumPy + oracle restatement
(tests/cloud_continuous_ref.py), alone and accumulated into edge_continuous's result; the special cases; graph capture across a cloud
update; soundness against dense sampling and on a wall of points that sampled checks step through; the connector and PRM.  Needs a real
MI355X.

The mixed-verdict conditions (at least 10 FREE and 10 COLLISION edges, at most a quarter UNDECIDED + DEGENERATE, a +inf exit, a D_cap
exit at look_ahead 0.03) are asserted on the RESTATEMENT for every scene's batch of 130 edges against its cloud of 200 points.  A cloud
of ONE point of radius 0.01 cannot block 10 of 130 random edges (the best of 60 draws blocks 4): its batches must hold a COLLISION, 10
FREE edges and both exits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd.scenes import build_scene
from test_gpu_parity import torch_cuda      # noqa: F401  (fixture)
from cloud_cases import scan, cloud_model, cloud_mask
from continuous_ref import random_edges, reference_continuous, thin_plate_scene, tree_scene, FREE, COLLISION, UNDECIDED, DEGENERATE
from cloud_continuous_ref import (reference_cloud_continuous, dense_cloud_min_distance, plate_wall, selection, EXIT_INF, EXIT_CAP)

R = 0.01
BOX = ([-0.6, -0.6, 0.0], [0.6, 0.6, 1.0])
INF = float("inf")
# scene -> how it is built, the threshold, where its scan stands (scan * f + (0, 0, dz): the tree gripper is a small machine), the
# length of its edges and the seed of its one-point scan -- all chosen on the CPU with the restatement alone
CASES = {
    "c2": dict(scene="c2", margins=True, thr=0.0, f=1.0, dz=0.0, scale=0.15, one=49),
    "c2m": dict(scene="c2m", margins=False, thr=0.0, f=1.0, dz=0.0, scale=0.15, one=49),
    "c2m-neg": dict(scene="c2m", margins=False, thr=-0.005, f=1.0, dz=0.0, scale=0.15, one=49),
    "tree": dict(scene="tree", margins=True, thr=0.0, f=0.5, dz=0.2, scale=0.3, one=39),
}
# (mode, dist given, look_ahead, shapes: "arm" = all but the base, which stands on the scanned table; "sub" = the last three)
CONFIGS = [("connect", False, 0.03, "arm"), ("steer", False, INF, "arm"), ("steer", True, 0.03, "sub"), ("connect", True, INF, "sub")]
STEER_MAXD = 0.4


def _build(case):
    c = CASES[case]
    return tree_scene() if c["scene"] == "tree" else build_scene(c["scene"], bullet_margins=c["margins"])


def case_points(case, N):
    c = CASES[case]
    return np.ascontiguousarray(scan(N, seed=N if N > 1 else c["one"]) * c["f"] + np.array([0.0, 0.0, c["dz"]]))


def case_edges(case, chain):
    """128 random edges and two degenerate ones."""
    s, g = random_edges(chain, 128, 31, scale=CASES[case]["scale"])
    return np.concatenate((s, s[:2])), np.concatenate((g, s[:2] + 1e-9))


def shape_sets(sm):
    return {"arm": list(range(1, sm.n_rshapes)), "sub": list(range(sm.n_rshapes - 3, sm.n_rshapes)), "all": None}


def given_dist(s, g):
    return 1.1 * np.linalg.norm(g - s, axis=1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _assert_same(dev, ref, what, n=None):
    v, end, tf, st = (_host(x) for x in dev)
    rv, rend, rtf, rst = (a if n is None else a[:n] for a in ref[:4])
    assert np.array_equal(v.astype(bool), rv), f"{what}: valid differs on {np.nonzero(v.astype(bool) != rv)[0][:10]}"
    assert np.array_equal(st, rst), f"{what}: status differs on {np.nonzero(st != rst)[0][:10]}: {st[st != rst][:10]} vs {rst[st != rst][:10]}"
    assert np.array_equal(_bits(tf), _bits(rtf)), f"{what}: t_free differs on {np.nonzero(_bits(tf) != _bits(rtf))[0][:10]}"
    assert np.array_equal(_bits(end), _bits(rend)), f"{what}: end differs"


def check_mixture(ref, what, look_ahead, one_point=False):
    """The conditions on the inputs, asserted on the restatement's output."""
    st, exits = ref[3], ref[6]
    n_free, n_col = int((st == FREE).sum()), int((st == COLLISION).sum())
    n_rest = int((st == UNDECIDED).sum() + (st == DEGENERATE).sum())
    assert n_free >= 10, f"{what}: {n_free} FREE edges"
    assert n_col >= (1 if one_point else 10), f"{what}: {n_col} COLLISION edges"
    if not one_point:
        assert 4 * n_rest <= st.shape[0], f"{what}: {n_rest} UNDECIDED or DEGENERATE edges of {st.shape[0]}"
    assert exits[EXIT_INF] >= 1, f"{what}: no item takes the +inf exit"
    if look_ahead != INF:
        assert exits[EXIT_CAP] >= 1, f"{what}: no item takes the D_cap exit"
    else:
        assert exits[EXIT_CAP] == 0


def linear_references(case, sm, chain, N):
    """[(config, reference)] of the case's batch against its cloud of N points; N = 1 runs the first two configs with every shape."""
    s, g = case_edges(case, chain)
    pts = case_points(case, N)
    sets = shape_sets(sm)
    out = []
    for mode, given, la, which in (CONFIGS if N > 1 else [(m, d, la, "all") for m, d, la, _ in CONFIGS[:2]]):
        maxd = STEER_MAXD if mode == "steer" else 10.0
        dist = given_dist(s, g) if given else None
        ref = reference_cloud_continuous(sm, pts, R, s, g, maxd, mode=mode, threshold=CASES[case]["thr"], look_ahead=la, dist=dist,
                                         shapes=sets[which])
        out.append(((mode, given, la, which, maxd, dist), ref))
    return s, g, pts, out


# ---- 1. linear edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_linear_edges_equal_the_restatement(fresh_world, case, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = _build(case)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    sets = shape_sets(sm)
    thr = CASES[case]["thr"]
    for N in (200, 1):
        s, g, pts, refs = linear_references(case, sm, chain, N)
        cloud = PointCloud(pts, R, bounds=BOX)
        for k, ((mode, given, la, which, maxd, dist), ref) in enumerate(refs):
            what = f"{case} N={N} {mode} dist={'given' if given else 'None'} look_ahead={la} shapes={which}"
            if which != "sub":
                check_mixture(ref, what, la, one_point=N == 1)
            if mode == "steer":
                live = ref[3] != DEGENERATE
                assert (_bits(ref[1][live]) != _bits(g[live])).any(), f"{what}: no edge is clipped by max_distance"
            assert (ref[3][-2:] == DEGENERATE).all()
            for E in ((1, 63, 65, 130) if k == 0 else (130,)):
                got = dev.cloud_edge_continuous(cloud, s[:E], g[:E], maxd, mode=mode, threshold=thr, look_ahead=la,
                                                dist=None if dist is None else dist[:E], shapes=sets[which])
                assert got[0].dtype == bool and got[3].dtype == np.int32
                _assert_same(got, ref, f"{what} E={E}", E)


# ---- 2. accumulate ----------------------------------------------------------------------------------------------------------------
def accumulate_inputs(chain):
    s, g = random_edges(chain, 128, 31, scale=0.15)
    return np.concatenate((s, s[:2])), np.concatenate((g, s[:2] + 1e-9))


def test_accumulate_is_one_call_over_scene_and_cloud(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.engine import DeviceModel
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    orc = Oracle(sm)
    _, dev = arm._scene_device()
    shapes = shape_sets(sm)["arm"]
    pts = case_points("c2", 200)
    cloud = PointCloud(pts, R, bounds=BOX)
    s, g = accumulate_inputs(chain)
    st_, gt_ = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    for mode, la in (("connect", 0.03), ("steer", INF)):
        maxd = STEER_MAXD if mode == "steer" else 10.0
        own = reference_continuous(sm, orc, s, g, maxd, mode=mode)
        only = reference_cloud_continuous(sm, pts, R, s, g, maxd, mode=mode, look_ahead=la, shapes=shapes)
        both = reference_cloud_continuous(sm, pts, R, s, g, maxd, mode=mode, look_ahead=la, shapes=shapes, scene_orc=orc)
        assert ((own[3] != FREE) & (only[3] == FREE)).sum() >= 3 and ((own[3] == FREE) & (only[3] != FREE)).sum() >= 3, \
            "each side must stop edges of its own"
        assert (both[3] == FREE).sum() >= 10
        valid, end, t_free, status = dev.edge_continuous(st_, gt_, maxd, mode=mode)
        _assert_same((valid, end, t_free, status), own, f"scene alone {mode}")
        t_scene = t_free.clone()
        got = dev.cloud_edge_continuous(cloud, st_, gt_, maxd, mode=mode, look_ahead=la, shapes=shapes, out=(valid, t_free, status))
        assert got[0] is valid and got[2] is t_free and got[3] is status
        _assert_same(got, both, f"accumulated {mode} look_ahead={la}")
        assert np.array_equal(_bits(got[1].cpu().numpy()), _bits(end.cpu().numpy())), "the end states of the two calls"
        live = both[3] != DEGENERATE
        assert (t_free.cpu().numpy()[live] <= t_scene.cpu().numpy()[live]).all(), "an edge's stop point only ever moves down"
    for bad in ((valid, t_free), (valid[:5], t_free, status), (valid, t_free.float(), status), (valid, t_free, status.cpu()), valid):
        with pytest.raises(ValueError, match="out must be"):
            dev.cloud_edge_continuous(cloud, st_, gt_, 10.0, shapes=shapes, out=bad)


def test_accumulate_equals_the_descriptor_that_holds_the_points(fresh_world, torch_cuda):
    """edge_continuous + cloud_edge_continuous(out=...) against nbk_edge_continuous_batch on the descriptor that holds the cloud's
    points as sphere world shapes: per (shape, point) pair there, per shape here -- the same verdicts, and the same stop point where
    both stop at T_f or at the start."""
    from numbotics_amd.engine import DeviceModel
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    orc = Oracle(sm)
    _, dev = arm._scene_device()
    shapes = [sm.n_rshapes - 2, sm.n_rshapes - 1]
    pts = case_points("c2", 200)
    cloud = PointCloud(pts, R, bounds=BOX)
    s, g = accumulate_inputs(chain)
    s, g = s[-65:], g[-65:]
    both = reference_cloud_continuous(sm, pts, R, s, g, 10.0, look_ahead=INF, shapes=shapes, scene_orc=orc)
    assert (both[3] == FREE).sum() >= 10 and (both[3] == COLLISION).sum() >= 5 and (both[3] == DEGENERATE).sum() == 2
    import torch
    st_, gt_ = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    valid, end, t_free, status = dev.edge_continuous(st_, gt_, 10.0)
    got = dev.cloud_edge_continuous(cloud, st_, gt_, 10.0, look_ahead=INF, shapes=shapes, out=(valid, t_free, status))
    _assert_same(got, both, "accumulated")
    held = DeviceModel(cloud_model(sm, pts, R, shapes, keep_scene=True))
    hv, hend, htf, hst = held.edge_continuous(s, g, 10.0)
    assert np.array_equal(hv, both[0]), f"valid differs on {np.nonzero(hv != both[0])[0][:10]}"
    assert np.array_equal(hst, both[3]), f"status differs on {np.nonzero(hst != both[3])[0][:10]}"
    same_stop = (both[3] == FREE) | (both[2] == 0.0)
    assert same_stop.sum() >= 10
    assert np.array_equal(_bits(htf[same_stop]), _bits(both[2][same_stop]))
    assert np.array_equal(_bits(hend), _bits(both[1]))


# ---- 3. special cases -------------------------------------------------------------------------------------------------------------
def test_special_cases(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = shape_sets(sm)["arm"]
    pts = case_points("c2", 200)
    s, g = case_edges("c2", chain)
    s, g = s[-65:].copy(), g[-65:].copy()                        # the two degenerate edges are the last ones
    ref = reference_cloud_continuous(sm, pts, R, s, g, 10.0, look_ahead=0.03, shapes=shapes)
    assert (ref[3] == FREE).sum() >= 5 and (ref[3] == COLLISION).sum() >= 5
    live = ref[3] != DEGENERATE
    assert live.sum() == 63
    free = (live, ref[1], np.where(live, 1.0, np.nan), np.where(live, FREE, DEGENERATE).astype(np.int32))
    cloud = PointCloud(pts, R, bounds=BOX)
    _assert_same(dev.cloud_edge_continuous(cloud, s, g, 10.0, look_ahead=0.03, shapes=[]), free, "empty selection")
    empty = PointCloud(np.zeros((0, 3)), R, bounds=BOX, capacity=8)
    _assert_same(dev.cloud_edge_continuous(empty, s, g, 10.0, look_ahead=0.03, shapes=shapes), free, "empty cloud")
    # a non-finite end point: every item of the edge is UNDECIDED at t = 0 (a NaN start with dist given; a NaN goal: 0 * NaN)
    s2, g2 = s.copy(), g.copy()
    dist = np.linalg.norm(g - s, axis=1)
    s2[3, 1] = np.nan
    g2[5, 0] = np.inf
    ref2 = reference_cloud_continuous(sm, pts, R, s2, g2, 10.0, look_ahead=0.03, shapes=shapes, dist=dist)
    for e in (3, 5):
        assert ref2[3][e] == UNDECIDED and ref2[2][e] == 0.0 and not ref2[0][e]
    _assert_same(dev.cloud_edge_continuous(cloud, s2, g2, 10.0, look_ahead=0.03, shapes=shapes, dist=dist), ref2, "non-finite end points")
    # a NaN point: every non-degenerate edge UNDECIDED with a NaN t_free, until a clean update
    bad = pts.copy()
    bad[123, 1] = np.nan
    cloud.update(bad)
    assert cloud.status() == 2
    unknown = (np.zeros(65, dtype=bool), ref[1], np.full(65, np.nan), np.where(live, UNDECIDED, DEGENERATE).astype(np.int32))
    _assert_same(dev.cloud_edge_continuous(cloud, s, g, 10.0, look_ahead=0.03, shapes=shapes), unknown, "status set")
    # ... also accumulating, whatever came in
    st_, gt_ = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    out = dev.edge_continuous(st_, gt_, 10.0)
    dev.cloud_edge_continuous(cloud, st_, gt_, 10.0, look_ahead=0.03, shapes=shapes, out=(out[0], out[2], out[3]))
    _assert_same(out, unknown, "status set, accumulating")
    cloud.update(pts)
    assert cloud.status() == 0
    # an edge that comes in with a NaN t_free keeps 0 / UNDECIDED / NaN; the others are reduced as usual
    scene = reference_cloud_continuous(sm, np.zeros((0, 3)), R, s, g, 10.0, shapes=shapes, scene_orc=Oracle(sm))
    both = reference_cloud_continuous(sm, pts, R, s, g, 10.0, look_ahead=0.03, shapes=shapes, scene_orc=Oracle(sm))
    out = dev.edge_continuous(st_, gt_, 10.0)
    _assert_same(out, scene, "the scene alone")
    keep = int(np.nonzero(both[3] == COLLISION)[0][0])
    out[0][keep], out[2][keep], out[3][keep] = False, float("nan"), UNDECIDED
    dev.cloud_edge_continuous(cloud, st_, gt_, 10.0, look_ahead=0.03, shapes=shapes, out=(out[0], out[2], out[3]))
    want = [a.copy() for a in both[:4]]
    want[0][keep], want[2][keep], want[3][keep] = False, np.nan, UNDECIDED
    _assert_same(out, want, "a NaN t_free coming in")
    _assert_same(dev.cloud_edge_continuous(cloud, s, g, 10.0, look_ahead=0.03, shapes=shapes), ref, "after a clean update")
    with pytest.raises(Exception, match="NBK_ERR_INVALID"):
        dev.cloud_edge_continuous(cloud, s, g, 10.0, look_ahead=0.0, shapes=shapes)


# ---- 4. capture -------------------------------------------------------------------------------------------------------------------
def test_graph_replay_reads_the_cloud_on_the_device(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = shape_sets(sm)["arm"]
    s, g = case_edges("c2", chain)
    s, g = s[-65:], g[-65:]
    first, other = case_points("c2", 200), np.ascontiguousarray(scan(120, seed=5))
    st_, gt_ = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    cloud = PointCloud(first, R, bounds=BOX, capacity=256)

    def run():
        valid, end, t_free, status = dev.edge_continuous(st_, gt_, 10.0)
        dev.cloud_edge_continuous(cloud, st_, gt_, 10.0, look_ahead=0.03, shapes=shapes, out=(valid, t_free, status))
        return valid, end, t_free, status
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                      # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = run()
    torch.cuda.current_stream().wait_stream(side)
    cloud.update(other)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    eager = run()
    torch.cuda.synchronize()
    ref_first = reference_cloud_continuous(sm, first, R, s, g, 10.0, look_ahead=0.03, shapes=shapes, scene_orc=Oracle(sm))
    ref_other = reference_cloud_continuous(sm, other, R, s, g, 10.0, look_ahead=0.03, shapes=shapes, scene_orc=Oracle(sm))
    assert (ref_first[3] != ref_other[3]).sum() >= 3, "the two scans must differ in their verdicts"
    _assert_same(out, ref_other, "replay after the update")
    _assert_same(out, [_host(x) for x in eager], "replay against the eager call")


# ---- 5. soundness -----------------------------------------------------------------------------------------------------------------
def test_free_edges_are_free_in_a_dense_sampling(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = shape_sets(sm)["sub"]
    pts = case_points("c2", 200)
    cloud = PointCloud(pts, R, bounds=BOX)
    s, g = case_edges("c2", chain)
    s, g = s[:24], g[:24]
    for thr, la in ((0.0, 0.03), (0.01, INF)):
        valid, end, t_free, status = dev.cloud_edge_continuous(cloud, s, g, 10.0, threshold=thr, look_ahead=la, shapes=shapes)
        assert valid.sum() >= 5 and (~valid).sum() >= 3
        for e in np.nonzero(valid)[0]:
            d = dense_cloud_min_distance(sm, pts, R, shapes, s[e], g[e], n=2000)
            assert d > thr, f"edge {e} certified free at threshold {thr}, but a dense sample is at {d}"


def grazing_edges(dev, cloud, shapes, s, g, n=2000, longest=0.045):
    """Edges that cross the cloud in less than one sampling step: every edge s -> g is sampled at n + 1 points (cloud_validity);
    each run of colliding samples with a free sample on either side, those two no further apart than ``longest`` in joint space,
    gives the edge from the one free sample to the other."""
    t = np.linspace(0.0, 1.0, n + 1)
    A, B = [], []
    for e in range(s.shape[0]):
        q = (1.0 - t)[:, None] * s[e] + t[:, None] * g[e]
        hit = np.asarray(dev.cloud_validity(cloud, q, 0.0, shapes=shapes))
        edge = np.flatnonzero(np.diff(hit.astype(np.int8)))            # sample i differs from sample i + 1
        for a, b in zip(edge[:-1], edge[1:]):
            if not hit[a] and hit[a + 1] and not hit[b + 1] and np.linalg.norm(q[b + 1] - q[a]) <= longest:
                A.append(q[a]); B.append(q[b + 1])
    return np.array(A), np.array(B)


def test_a_wall_of_points_is_not_stepped_through(fresh_world, torch_cuda):
    """A wall of overlapping spheres on the plane of the thin plate.  The random edges that cross it (rejected by the sampled check at
    resolution 0.001) are not certified.  Edges that cross it in less than 0.05 of joint-space length -- cut out of the random
    ones around their shortest contacts -- are all accepted by the sampled check at resolution 0.05, which looks at their two end
    points only, and none is certified."""
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = thin_plate_scene()
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = shape_sets(sm)["arm"]
    wall = plate_wall(0.015)
    d = np.linalg.norm(wall[:, None, 1:] - wall[None, :60, 1:], axis=2)
    assert wall.shape[0] > 2000 and np.sort(d, axis=0)[1].max() < 2 * R, "neighbouring spheres overlap"
    cloud = PointCloud(wall, R, bounds=BOX)
    s, g = random_edges(chain, 400, 5, scale=0.4)
    keep = ~dev.cloud_validity(cloud, s, 0.0, shapes=shapes) & ~dev.cloud_validity(cloud, g, 0.0, shapes=shapes)
    s, g = s[keep], g[keep]
    fine = dev.cloud_edge_validity(cloud, s, g, 0.001, 10.0, shapes=shapes)[0]
    crossing = ~fine
    assert crossing.sum() >= 10
    valid, _, _, status = dev.cloud_edge_continuous(cloud, s, g, 10.0, shapes=shapes)
    assert not (valid & crossing).any(), f"certified free through the wall: edges {np.nonzero(valid & crossing)[0][:8]}"
    assert valid.any(), "the certified check accepts nothing at all"
    A, B = grazing_edges(dev, cloud, shapes, s[crossing], g[crossing])
    print(f"{int(crossing.sum())} crossing edges of {s.shape[0]}, {A.shape[0]} contacts shorter than a step")
    assert A.shape[0] >= 3, "no edge crosses the wall between two samples 0.05 apart"
    coarse, _, ns = dev.cloud_edge_validity(cloud, A, B, 0.05, 10.0, shapes=shapes)
    assert (ns == 2).all() and coarse.all(), "the sampled check at resolution 0.05 looks at the end points, which are free"
    valid, _, _, status = dev.cloud_edge_continuous(cloud, A, B, 10.0, shapes=shapes)
    assert not valid.any(), f"certified free through the wall: {np.nonzero(valid)[0][:8]}"      # (a graze this shallow ends UNDECIDED)


# ---- 6. the connector -------------------------------------------------------------------------------------------------------------
def connector_inputs(chain):
    s, g = random_edges(chain, 64, 31, scale=0.15)
    return s, g


def prm_samples(chain, n=14):
    rng = np.random.default_rng(3)
    start, goal = np.zeros(chain.dof), np.full(chain.dof, 0.3)
    samples = [start + rng.normal(0.0, 0.8, chain.dof) for _ in range(n)]
    return start, goal, samples


def test_connector_and_prm_with_a_cloud(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    from numbotics_amd.planning.sampling_based import ConnectorParams, ContinuousConnector, EuclideanSpace, PlannerParams, PRM
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    orc = Oracle(sm)
    pts = case_points("c2", 200)
    cloud = PointCloud(pts, R, bounds=BOX)
    base = sm.links[sm.rshape_link[0]]._name
    shapes = [k for k in range(sm.n_rshapes) if sm.links[sm.rshape_link[k]]._name != base]
    assert 0 < len(shapes) < sm.n_rshapes
    la = 0.05
    cp = ConnectorParams(max_distance=STEER_MAXD, arm=arm)
    cc = ContinuousConnector(cp, cloud=cloud, cloud_ignore_links=(base,), look_ahead=la)
    plain = ContinuousConnector(cp)
    s, g = connector_inputs(chain)
    dist = np.array([np.linalg.norm(s[e] - g[e]) for e in range(s.shape[0])])      # what connect / steer pass for one edge
    both = {m: reference_cloud_continuous(sm, pts, R, s, g, STEER_MAXD, mode=m, look_ahead=la, shapes=shapes, scene_orc=orc, dist=dist)
            for m in ("connect", "steer")}
    own = {m: reference_continuous(sm, orc, s, g, STEER_MAXD, mode=m, dist=dist) for m in ("connect", "steer")}
    for m in both:
        assert (both[m][3] == FREE).sum() >= 10 and (own[m][0] & ~both[m][0]).sum() >= 3, "the cloud must stop edges the scene lets through"
        _assert_same(cc.certify_batch(s, g, m, dist), both[m], f"certify_batch {m}")
        _assert_same(plain.certify_batch(s, g, m, dist), own[m], f"certify_batch {m} without a cloud")
    ok = cc.connect_batch(s, g, dist)
    assert ok.dtype == bool and np.array_equal(ok, both["connect"][0])
    ok, end = cc.steer_batch(s, g, dist)
    assert np.array_equal(ok, both["steer"][0]) and np.array_equal(_bits(end), _bits(both["steer"][1]))
    ref = both["connect"][0]
    for e in np.concatenate((np.flatnonzero(ref)[:3], np.flatnonzero(~ref)[:3])):
        out = cc.connect(s[e], g[e])
        assert (out is not None) == bool(ref[e]), f"connect, edge {e}"
        if out is not None:
            assert np.array_equal(_bits(out), _bits(g[e]))
        out = cc.steer(s[e], g[e])
        assert (out is not None) == bool(both["steer"][0][e]), f"steer, edge {e}"
        if out is not None:
            assert np.array_equal(_bits(out), _bits(both["steer"][1][e]))
    q = np.concatenate((s[:8], g[:8]))
    hit = orc.validity(q) | cloud_mask(sm, pts, R, q, 0.0, shapes)
    assert hit.any() and (~hit).any()
    assert np.array_equal(np.array([cc.is_valid(x) for x in q]), ~hit)
    with pytest.raises(ValueError, match="do not see point clouds yet"):
        cc.validate_trajectories(np.stack((s[:4], g[:4]), axis=1), degree=1)
    # PRM accepts exactly the edges the restatement accepts
    lim = np.asarray(chain.joint_limits, dtype=np.float64)
    lim = np.where(np.isfinite(lim), lim, np.sign(lim) * np.pi)
    space = EuclideanSpace(lim[:, 0], lim[:, 1])
    start, goal, samples = prm_samples(chain)
    prm = PRM(space, ContinuousConnector(ConnectorParams(max_distance=2.0, arm=arm), cloud=cloud, cloud_ignore_links=(base,), look_ahead=la),
              PlannerParams(max_iters=len(samples), k_nearest=4, goal_bias=0.0))
    prm.add_start(start)
    prm.add_goal(goal)
    V, nodes, cand, cdist = prm.candidate_edges(samples)
    live = cdist > np.finfo(np.float32).eps
    want = np.zeros(cand.shape[0], dtype=bool)
    want[live] = reference_cloud_continuous(sm, pts, R, nodes[cand[live, 0]], nodes[cand[live, 1]], 2.0, look_ahead=la, shapes=shapes,
                                            scene_orc=orc, dist=cdist[live])[0]
    assert want.sum() >= 3 and (~want).sum() >= 3
    prm.plan(samples)
    assert prm.n_candidate_edges == cand.shape[0]
    assert {(int(a), int(b)) for a, b in prm.edges} == {(int(a), int(b)) for a, b in cand[want]}
