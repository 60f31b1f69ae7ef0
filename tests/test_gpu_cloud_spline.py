"""Sampled B-spline trajectories against a point cloud on the device (nbk_spline_cloud_validity_batch,
DeviceModel.cloud_spline_validity, DiscreteConnector.validate_trajectories(..., cloud=...)): valid / t_hit / n_samples bit-identical to
the NumPy + oracle restatement (tests/cloud_spline_ref.py) over the degrees, control counts, cloud sizes and selections; the flat
sample range at its edges (a total that is no multiple of 64, trajectories without samples first, in the middle and last, repeated
knots, a trajectory of too many samples, a total beyond one pass of the fixed grid); the accumulate form against
nbk_spline_validity_batch on the descriptor that holds the points; the two-point linear spline against the edge entry; the cloud's
status; graph capture across a cloud update; the connector's keyword.  Needs a real MI355X.

Every condition on the inputs (a valid and an invalid trajectory in each batch, t_hit going down and staying, the sample totals) is
asserted on the RESTATEMENT; the seeds were chosen on the CPU with it alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd.planning import unit_bspline, unit_knots
from numbotics_amd.scenes import build_scene
from test_gpu_parity import torch_cuda      # noqa: F401  (fixture)
from test_gpu_cloud_continuous import CASES, BOX, R, _build, case_points, case_edges, shape_sets
from cloud_cases import cloud_model, cloud_mask
from spline_ref import random_splines, reference_splines, speed_bound
from cloud_spline_ref import reference_cloud_splines, merge_scene_and_cloud

RES = 0.05
SCENES = ["c2", "tree"]
# (case, degree) -> the seed of its trajectories: the first one, counting up from 1000 * degree, for which every batch of the case
# against 1 and against 200 points holds a valid and an invalid trajectory in the restatement
SEEDS = {("c2", 1): 1004, ("c2", 2): 2008, ("c2", 3): 3004, ("c2", 4): 4036, ("c2", 5): 5020,
         ("tree", 1): 1001, ("tree", 2): 2000, ("tree", 3): 3000, ("tree", 4): 4000, ("tree", 5): 5000}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _assert_same(got, ref, what):
    v, th, ns = (_host(x) for x in got)
    rv, rth, rns = ref[:3]
    assert np.array_equal(ns, rns), f"{what}: n_samples differs on {np.nonzero(ns != rns)[0][:10]}"
    assert np.array_equal(v.astype(bool), rv), f"{what}: valid differs on {np.nonzero(v.astype(bool) != rv)[0][:10]}"
    assert np.array_equal(_bits(th), _bits(rth)), f"{what}: t_hit differs on {np.nonzero(_bits(th) != _bits(rth))[0][:10]}"


def free_q(case, sm, chain):
    """A configuration clear of the scene and, but for the base (it stands on the scanned table), of the case's scan of 200 points."""
    q = random_splines(chain, 2000, 2, 5)[:, 0] * (0.3 if case == "c2" else 1.0)      # (near its zero the tree gripper sits in its scan's table)
    ok = ~Oracle(sm).validity(q, CASES[case]["thr"]) & ~cloud_mask(sm, case_points(case, 200), R, q, CASES[case]["thr"], shape_sets(sm)["arm"])
    return q[ok][0]


def parity_batches(case, sm, chain, k, seed):
    """[(n, trajectories, N, shapes name)] of one (case, degree): n in {k + 1, k + 3, 9}, 24 trajectories each, half over the joint
    box and half within 0.05 / 0.3 of a free configuration; every n against 0, 1 and 200 points, the selection alternating between
    every shape (None) and a subset -- against 200 points between two subsets: the base stands on the scanned table."""
    free = free_q(case, sm, chain)
    out = []
    for i, n in enumerate(sorted({k + 1, k + 3, 9})):
        c = random_splines(chain, 24, n, seed + n, near=free, spread=(0.05, 0.3)[(i + k) % 2])
        for j, N in enumerate((0, 1, 200)):
            out.append((n, c, N, (("arm", "sub") if N == 200 else ("arm", "all"))[(i + j) % 2]))
    return out


def batches_are_mixed(case, sm, batches, k):
    """The restatement's results of the batches, or None when one with points lacks a valid or an invalid trajectory."""
    refs = []
    for n, c, N, which in batches:
        ref = reference_cloud_splines(sm, case_points(case, N), R, c, unit_knots(n, k), k, RES, CASES[case]["thr"], shape_sets(sm)[which])
        if N > 0 and not (ref[0].any() and (~ref[0]).any()):
            return None
        refs.append(ref)
    return refs


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("case", SCENES)
def test_bit_parity_with_the_restatement(fresh_world, case, k, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = _build(case)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    batches = parity_batches(case, sm, chain, k, SEEDS[case, k])
    refs = batches_are_mixed(case, sm, batches, k)
    assert refs is not None, "a batch against points holds no valid or no invalid trajectory"
    clouds = {N: PointCloud(case_points(case, N), R, bounds=BOX, capacity=256) for N in (0, 1, 200)}
    for (n, c, N, which), ref in zip(batches, refs):
        got = dev.cloud_spline_validity(clouds[N], c, unit_knots(n, k), k, RES, threshold=CASES[case]["thr"], shapes=shape_sets(sm)[which])
        assert got[0].dtype == bool and got[2].dtype == np.int32
        _assert_same(got, ref, f"{case} k={k} n={n} N={N} shapes={which}")
        if N == 0:
            assert np.array_equal(got[0], got[2] > 0), "an empty cloud leaves every trajectory with samples valid"


# ---- 2. the edges of the flat sample range ------------------------------------------------------------------------------------------
def boundary_trajectories(chain, free, kn):
    """9 trajectories of 7 control points: all control points equal first, in the middle and last, a NaN control point, one of more
    than 2^32 samples and one of between 2^31 and 2^32 at RES on the knots kn; the rest ordinary ones."""
    c = random_splines(chain, 9, 7, 91, near=free, spread=0.3)
    c[0] = free
    c[4] = c[4, 0]
    c[8] = free
    c[2, 3, 1] = np.nan
    for s, inv in ((5, 1e12), (6, 3e9)):                 # 1 / step = V / RES
        c[s] = free + (c[s] - free) * (inv * RES / speed_bound(c[s], kn, 3))
    return c


def test_the_flat_sample_range_at_its_edges(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = shape_sets(sm)["arm"]
    free = free_q("c2", sm, chain)
    pts = case_points("c2", 200)
    cloud = PointCloud(pts, R, bounds=BOX)
    for kn in (unit_knots(7, 3), np.array([0.0, 0.0, 0.0, 0.0, 0.4, 0.4, 0.7, 1.0, 1.0, 1.0, 1.0])):      # ... and a repeated interior knot
        c = boundary_trajectories(chain, free, kn)
        ref = reference_cloud_splines(sm, pts, R, c, kn, 3, RES, 0.0, shapes)
        assert list(ref[2][[0, 2, 4, 8]]) == [0, 0, 0, 0] and list(ref[2][[5, 6]]) == [-1, -1] and (ref[2][[1, 3, 7]] > 0).all()
        assert int(ref[2][[1, 3, 7]].sum()) % 64 != 0, "the live samples must not fill whole waves"
        assert not ref[0][[0, 2, 4, 5, 6, 8]].any() and np.isnan(ref[1][[0, 2, 4, 5, 6, 8]]).all()
        _assert_same(dev.cloud_spline_validity(cloud, c, kn, 3, RES, shapes=shapes), ref, "boundaries")
    # a few live trajectories alone, each count of them: the total is no multiple of 64 either way
    live = c[[1, 3, 7]]
    ref = reference_cloud_splines(sm, pts, R, live, unit_knots(7, 3), 3, RES, 0.0, shapes)
    assert ref[0].any() and (~ref[0]).any()
    for S in (1, 2, 3):
        assert int(ref[2][:S].sum()) % 64 != 0
        _assert_same(dev.cloud_spline_validity(cloud, live[:S], unit_knots(7, 3), 3, RES, shapes=shapes), [a[:S] for a in ref], f"S={S}")
    # knots on the device that break the rules: every trajectory invalid, without samples
    for bad in (unit_knots(7, 3) * 2.0, np.where(unit_knots(7, 3) == 0.25, 0.8, unit_knots(7, 3)), np.where(unit_knots(7, 3) == 0.5, np.nan, unit_knots(7, 3))):
        v, th, ns = dev.cloud_spline_validity(cloud, c, bad, 3, RES, shapes=shapes)
        assert not v.any() and np.isnan(th).all() and (ns == 0).all()
        _assert_same((v, th, ns), reference_cloud_splines(sm, pts, R, c, bad, 3, RES, 0.0, shapes), "bad knots")


STRIDE_SEED = 4          # the first seed whose batch exceeds one pass and holds a valid and an invalid trajectory against the one point


def test_a_total_beyond_one_pass_of_the_grid(fresh_world, torch_cuda):
    """More samples than the fixed grid has lanes: the kernel's stride serves the rest.  One point keeps the oracle cheap."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    free = free_q("c2", sm, chain)
    pts = case_points("c2", 1)
    c = random_splines(chain, 24, 8, STRIDE_SEED, near=free, spread=0.3)
    ref = reference_cloud_splines(sm, pts, R, c, unit_knots(8, 3), 3, 0.002, 0.0, None)
    one_pass = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 64
    assert int(ref[2].sum()) > one_pass + 64, f"{int(ref[2].sum())} samples do not exceed one pass of {one_pass}"
    assert ref[0].any() and (~ref[0]).any()
    _assert_same(dev.cloud_spline_validity(PointCloud(pts, R, bounds=BOX), c, unit_knots(8, 3), 3, 0.002), ref, "stride")



# ---- 3. accumulate ----------------------------------------------------------------------------------------------------------------
ACC_SEED = 0             # the first seed that meets the conditions the accumulate, status, capture and connector tests assert


def accumulate_inputs(sm, chain):
    return random_splines(chain, 48, 8, ACC_SEED, near=free_q("c2", sm, chain), spread=0.3), unit_knots(8, 3), 3


def test_accumulate_is_the_descriptor_that_holds_scene_and_points(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd import _lib
    from numbotics_amd.engine import DeviceModel
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = shape_sets(sm)["arm"]
    pts = case_points("c2", 200)
    cloud = PointCloud(pts, R, bounds=BOX)
    c, kn, k = accumulate_inputs(sm, chain)
    scene = reference_splines(Oracle(sm), c, kn, k, RES)
    alone = reference_cloud_splines(sm, pts, R, c, kn, k, RES, 0.0, shapes)
    both = reference_cloud_splines(sm, pts, R, c, kn, k, RES, 0.0, shapes, prev=(scene[0], scene[1]))
    for a, b in zip(both, merge_scene_and_cloud(scene, alone)):
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
    hit = ~scene[0] & ~alone[0]
    with np.errstate(invalid="ignore"):
        assert (hit & (alone[1] < scene[1])).any(), "no trajectory the scene rejects late and the cloud hits earlier"
        assert (hit & (scene[1] < alone[1])).any(), "no trajectory the cloud hits late and the scene rejects earlier"
    assert (scene[0] & ~alone[0]).any() and both[0].any()
    ct = torch.from_numpy(c).cuda()
    out = dev.spline_validity(ct, kn, k, RES)
    _assert_same(out, scene, "the scene alone")
    t_scene = out[1].clone()
    got = dev.cloud_spline_validity(cloud, ct, kn, k, RES, shapes=shapes, out=out)
    assert all(a is b for a, b in zip(got, out))
    _assert_same(got, both, "accumulated")
    new, old = got[1].cpu().numpy(), t_scene.cpu().numpy()
    changed = _bits(new) != _bits(old)
    with np.errstate(invalid="ignore"):
        assert (changed & (new < old)).any(), "no t_hit went down"
        assert (np.isnan(old[changed]) | (new[changed] < old[changed])).all(), "a t_hit only ever appears or moves down"
    held = DeviceModel(cloud_model(sm, pts, R, shapes, keep_scene=True))
    _assert_same(held.spline_validity(c, kn, k, RES), both, "the descriptor that holds scene and points")
    # without t_hit: an entry that comes in 0 stays 0 and none of its samples is looked at; the others get the cloud's verdict
    lib = _lib.load()
    valid = torch.from_numpy(scene[0].astype(np.uint8)).cuda()
    knt = torch.from_numpy(kn).cuda()
    ws = torch.empty((dev.cloud_spline_workspace_bytes(48),), dtype=torch.uint8, device="cuda")
    bits = dev._shape_bits(shapes)
    _lib.check(lib.nbk_spline_cloud_validity_batch(dev._h, cloud._h, ct.data_ptr(), 48, 8, k, knt.data_ptr(), RES, 0.0, bits.ctypes.data, 1,
                                                   valid.data_ptr(), None, None, ws.data_ptr(), ws.numel(), None), "accumulate without t_hit")
    torch.cuda.synchronize()
    assert np.array_equal(valid.cpu().numpy().astype(bool), both[0])
    for bad in ((out[0], out[1]), (out[0][:5], out[1], out[2]), (out[0], out[1].float(), out[2]), (out[0], out[1], out[2].cpu()), out[0]):
        with pytest.raises(ValueError, match="out must be"):
            dev.cloud_spline_validity(cloud, ct, kn, k, RES, shapes=shapes, out=bad)


# ---- 4. the linear two-point spline ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SCENES)
def test_linear_spline_is_the_edge_entry(fresh_world, case, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = _build(case)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = shape_sets(sm)["arm"]
    cloud = PointCloud(case_points(case, 200), R, bounds=BOX)
    s, g = case_edges(case, chain)
    thr = CASES[case]["thr"]
    ok, _, ns = dev.cloud_edge_validity(cloud, s, g, RES, 1e9, mode="connect", threshold=thr, shapes=shapes)
    v, th, sns = dev.cloud_spline_validity(cloud, np.stack((s, g), axis=1), unit_knots(2, 1), 1, RES, threshold=thr, shapes=shapes)
    assert np.array_equal(sns, ns) and np.array_equal(v, ok)
    assert (sns[-2:] == 0).all() and not v[-2:].any() and 0 < v.sum() < v.shape[0] - 2
    assert np.isnan(th[v]).all() and not np.isnan(th[~v & (sns > 0)]).any()
    _assert_same((v, th, sns), reference_cloud_splines(sm, case_points(case, 200), R, np.stack((s, g), axis=1), unit_knots(2, 1), 1, RES, thr,
                                                       shapes), "two-point splines")


# ---- 5. the cloud's status ------------------------------------------------------------------------------------------------------
def test_status_set_and_recovery(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = shape_sets(sm)["arm"]
    pts = case_points("c2", 200)
    c, kn, k = accumulate_inputs(sm, chain)
    c = c[14:34].copy()                                  # ten over the joint box, ten near the free configuration
    c[7] = c[7, 0]                                       # one degenerate trajectory
    ref = reference_cloud_splines(sm, pts, R, c, kn, k, RES, 0.0, shapes)
    assert ref[0].any() and (~ref[0]).any() and ref[2][7] == 0
    cloud = PointCloud(pts, R, bounds=BOX)
    bad = pts.copy()
    bad[123, 1] = np.nan
    cloud.update(bad)
    assert cloud.status() == 2
    blocked = reference_cloud_splines(sm, pts, R, c, kn, k, RES, 0.0, shapes, status=2)
    live = ref[2] > 0
    assert not blocked[0].any() and (blocked[1][live] == 0.0).all() and np.isnan(blocked[1][7]) and np.array_equal(blocked[2], ref[2])
    _assert_same(dev.cloud_spline_validity(cloud, c, kn, k, RES, shapes=shapes), blocked, "status set")
    # ... also accumulating, whatever came in
    ct = torch.from_numpy(c).cuda()
    out = dev.spline_validity(ct, kn, k, RES)
    _assert_same(dev.cloud_spline_validity(cloud, ct, kn, k, RES, shapes=shapes, out=out), blocked, "status set, accumulating")
    cloud.update(pts)
    assert cloud.status() == 0
    _assert_same(dev.cloud_spline_validity(cloud, c, kn, k, RES, shapes=shapes), ref, "after a clean update")
    _assert_same(dev.cloud_spline_validity(cloud, c, kn, k, RES, shapes=[]), (live, np.full(20, np.nan), ref[2]), "empty selection")


# ---- 6. capture -------------------------------------------------------------------------------------------------------------------
def test_graph_replay_reads_the_cloud_on_the_device(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = shape_sets(sm)["arm"]
    c, kn, k = accumulate_inputs(sm, chain)
    first, other = case_points("c2", 200), case_points("c2", 1)
    ct, knt = torch.from_numpy(c).cuda(), torch.from_numpy(kn).cuda()
    cloud = PointCloud(first, R, bounds=BOX, capacity=256)
    scene = dev.spline_validity(ct, kn, k, RES)          # (synchronous: not part of the graph)

    def run():
        alone = dev.cloud_spline_validity(cloud, ct, knt, k, RES, shapes=shapes)
        out = tuple(x.clone() for x in scene)
        dev.cloud_spline_validity(cloud, ct, knt, k, RES, shapes=shapes, out=out)
        return alone, out
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                      # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            alone, out = run()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    ref_first = reference_cloud_splines(sm, first, R, c, kn, k, RES, 0.0, shapes)
    _assert_same(alone, ref_first, "replay")
    cloud.update(other)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    eager = run()
    torch.cuda.synchronize()
    ref_other = reference_cloud_splines(sm, other, R, c, kn, k, RES, 0.0, shapes)
    assert (ref_first[0] != ref_other[0]).sum() >= 3, "the two scans must differ in their verdicts"
    _assert_same(alone, ref_other, "replay after the update")
    _assert_same(alone, [_host(x) for x in eager[0]], "replay against the eager call")
    sc = tuple(_host(x) for x in scene)
    _assert_same(out, reference_cloud_splines(sm, other, R, c, kn, k, RES, 0.0, shapes, prev=(sc[0], sc[1])), "accumulating replay")
    _assert_same(out, [_host(x) for x in eager[1]], "accumulating replay against the eager call")


# ---- 7. the connector -------------------------------------------------------------------------------------------------------------
def test_discrete_connector_with_a_cloud(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    from numbotics_amd.planning.sampling_based import ConnectorParams, DiscreteConnector
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    pts = case_points("c2", 200)
    cloud = PointCloud(pts, R, bounds=BOX)
    base = sm.links[sm.rshape_link[0]]._name
    shapes = [i for i in range(sm.n_rshapes) if sm.links[sm.rshape_link[i]]._name != base]
    assert 0 < len(shapes) < sm.n_rshapes
    c, kn, k = accumulate_inputs(sm, chain)
    scene = reference_splines(Oracle(sm), c, kn, k, RES)
    want = merge_scene_and_cloud(scene, reference_cloud_splines(sm, pts, R, c, kn, k, RES, 0.0, shapes))
    assert want[0].any() and (scene[0] & ~want[0]).any()
    conn = DiscreteConnector(ConnectorParams(resolution=RES, arm=arm, cloud_ignore_links=(base,)))
    got = conn.validate_trajectories(c, degree=k, cloud=cloud)
    assert isinstance(got[0], np.ndarray) and got[0].dtype == bool and got[2].dtype == np.int32
    _assert_same(got, want, "connector")
    dev_out = conn.validate_trajectories(torch.from_numpy(c).cuda(), degree=k, cloud=cloud)
    assert all(torch.is_tensor(x) and x.is_cuda for x in dev_out)
    _assert_same(dev_out, want, "connector, device tensors")
    _assert_same(conn.validate_trajectories(c, degree=k), scene, "connector without a cloud")
    every = merge_scene_and_cloud(scene, reference_cloud_splines(sm, pts, R, c, kn, k, RES, 0.0, None))
    _assert_same(conn.validate_trajectories(c, degree=k, cloud=cloud, cloud_ignore_links=()), every, "connector, no link ignored")
    for s in (int(np.flatnonzero(want[0])[0]), int(np.flatnonzero(~want[0] & scene[0])[0])):
        ok, t_hit = conn.validate_trajectory(unit_bspline(c[s], degree=k), cloud=cloud)
        assert ok == bool(want[0][s]) and _bits([t_hit])[0] == _bits(want[1])[s]
