"""Proximity records against a point cloud on the device (nbk_records_cloud_batch, DeviceModel.cloud_records,
Arm.cloud_proximity_jacobians / cloud_closest_to, safe_sets.cloud_distance_and_gradient): distance, shape, point, witness and
gradient row bit-identical to the CPU oracle run on the same robot with the cloud's points as sphere world shapes
(tests/cloud_records_cases.py), per configuration and per (configuration, shape), and to the sibling entry points.  Needs a real
MI355X.

Every mixed case asserts on the REFERENCE, before comparing, that between 5 % and 95 % of its configurations have a point nearer
than d_max and that a penetrating record is among them."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import assert_bitwise, torch_cuda      # noqa: F401  (fixture)
from test_gpu_cloud import _robot, _scan
from cloud_cases import cloud_model
from cloud_records_cases import Raw, cut

N = 300
RADII = (0.0, 0.01)
BATCHES = (1, 64, 65, 200)
# d_max = 0.05 is mixed for every robot here (the oracle on the CPU: 42-44 % of the configurations near on c1 and c2m, 70-74 % on
# the tree gripper with its scaled scan, 69-70 % on k9; 12-47 % of the (configuration, shape) items); at 0.5 every configuration is near
D_MIXED, D_ALL = 0.05, 0.5
# the clouds of the captured graph (other seeds of the scan): shape 1 stands 0.048-0.050 above the table's nearest point whatever q is,
# so 0.05 is mixed for seed 300 only; at 0.03 the oracle has 34-40 % of the configurations near for each of them
D_REPLAY = 0.03
ROBOTS = [("c1", True), ("c1", False), ("c2m", True), ("tree", True), ("k9", True)]
FIELDS = ("dist", "shape", "point", "witness", "rows")


def _points(name):
    """300 points of the scan with two duplicated points: the larger indices (299, 225) never win."""
    pts = _scan(name, N)
    pts[299] = pts[7]
    pts[150] = pts[225]
    return pts


def _same(got, ref, what, B=None):
    """Every field bit for bit (ints by value); ``ref`` cut to the first B rows."""
    for name, g, r in zip(FIELDS, got, ref):
        if g is None:
            continue
        r = r if B is None else r[:B]
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        if name in ("shape", "point"):
            assert g.dtype == np.int32 and g.shape == r.shape and np.array_equal(g, r), f"{what}: {name} differs at {np.argwhere(g != r)[:4].tolist()}"
        else:
            assert_bitwise(g, r, f"{what}: {name}")


def _mixed(ref, what):
    d = ref[0]
    share = np.isfinite(d).reshape(d.shape[0], -1).any(axis=1).mean()
    assert 0.05 <= share <= 0.95, f"{what}: {share:.3f} of the reference's configurations are near -- not a mixed case"
    assert (d[np.isfinite(d)] < 0).any(), f"{what}: no penetrating record in the reference"


@pytest.mark.parametrize("name,margins", ROBOTS, ids=[f"{n}-{'bullet' if m else 'sharp'}" for n, m in ROBOTS])
def test_records_bitwise(fresh_world, tmp_path, name, margins, torch_cuda):
    """c1: closed-form cores; c2m: hulls, per shape (a wave holds one hull: the scalar-cache path) and per configuration (the
    winners differ per lane: the vector path); tree: prismatic joints and branching masks; k9: the second trip of the q staging."""
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot(name, margins, tmp_path)
    q = q[:200]
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))                       # the base shape stands in the table's points
    pts = _points(name)
    for r in RADII:
        cloud = PointCloud(pts, r)
        raw = Raw(sm, pts, r, q, shapes)
        for d_max in (D_MIXED, D_ALL):
            for per_shape in (False, True):
                ref = cut(raw, d_max, per_shape)
                what = f"{name} r={r} d_max={d_max} per_shape={per_shape}"
                if d_max == D_MIXED:
                    _mixed(ref, what)
                elif not per_shape:
                    assert np.isfinite(ref[0]).all(), what
                assert not np.isnan(ref[3][np.isfinite(ref[0])]).any() and not np.isnan(ref[4]).any(), what
                assert not np.isin(ref[2], (299, 225)).any(), f"{what}: a duplicate's larger index won in the reference"
                for B in BATCHES:
                    _same(dev.cloud_records(cloud, q[:B], d_max, shapes=shapes, per_shape=per_shape), ref, f"{what} B={B}", B)
    # every shape, the base included (it stands in the table: deep penetration)
    raw = Raw(sm, pts, 0.01, q[:65])
    for per_shape in (False, True):
        _same(dev.cloud_records(PointCloud(pts, 0.01), q[:65], D_ALL, per_shape=per_shape), cut(raw, D_ALL, per_shape), f"{name} every shape")


@pytest.mark.parametrize("name", ["c1", "c2m"])
def test_records_agree_with_their_siblings(fresh_world, tmp_path, name, torch_cuda):
    from numbotics_amd.engine import DeviceModel
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot(name, True, tmp_path)
    q = q[:130]
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    pts = _points(name)
    r = 0.01
    cloud = PointCloud(pts, r)
    for d_max in (D_MIXED, D_ALL):
        d, s, p, w, j = dev.cloud_records(cloud, q, d_max, shapes=shapes)
        dc, sc, pc = dev.cloud_clearance(cloud, q, d_max, shapes=shapes)
        assert_bitwise(d, dc, f"{name} d_max={d_max}: distance against cloud_clearance")
        assert np.array_equal(s, sc) and np.array_equal(p, pc)
        # a per-shape column = the per-configuration call with that one shape selected = cloud_clearance of it
        per = dev.cloud_records(cloud, q, d_max, shapes=shapes, per_shape=True)
        assert per[0].shape == (130, len(shapes)) and per[3].shape == (130, len(shapes), 9) and per[4].shape == (130, len(shapes), sm.kin.n_q)
        for col, sh in enumerate(shapes):
            one = dev.cloud_records(cloud, q, d_max, shapes=[sh])
            _same([x[:, col] for x in per], one, f"{name} d_max={d_max}: column {col} against shape {sh} alone")
            assert_bitwise(one[0], dev.cloud_clearance(cloud, q, d_max, shapes=[sh])[0], f"{name}: shape {sh} alone against cloud_clearance")
    # across the seam: a descriptor that holds the winners' points as sphere world shapes; nbk_pair_records_items at (b, winning pair)
    d, s, p, w, j = dev.cloud_records(cloud, q, D_ALL, shapes=shapes)
    assert (s >= 0).all()
    uniq = np.unique(p)
    seam = DeviceModel(cloud_model(sm, pts[uniq], r, shapes))
    pair = np.searchsorted(np.asarray(shapes), s) * len(uniq) + np.searchsorted(uniq, p)
    items = np.stack((np.arange(130, dtype=np.int32), pair.astype(np.int32)), axis=1)
    ds, ws, js = seam.pair_records(q, items)
    assert_bitwise(d, ds, f"{name}: distance across the seam")
    assert_bitwise(w, ws, f"{name}: witness across the seam")
    assert_bitwise(j, js, f"{name}: rows across the seam")


def test_records_optional_outputs(fresh_world, tmp_path, torch_cuda):
    torch = torch_cuda
    from numbotics_amd import _lib
    from numbotics_amd.physics import PointCloud
    lib = _lib.load()
    arm, chain, keep, q = _robot("c2m", True, tmp_path)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    sets = [_scan("c2m", N)]
    qt = torch.from_numpy(q).cuda()
    for per_shape in (False, True):
        cloud = PointCloud(sets[0], 0.01)
        both = dev.cloud_records(cloud, qt, D_MIXED, shapes=shapes, per_shape=per_shape)
        assert all(torch.is_tensor(x) and x.is_cuda for x in both), "tensors in, tensors out"
        _same(both, cut(Raw(sm, sets[0], 0.01, q, shapes), D_MIXED, per_shape), f"tensor q per_shape={per_shape}")
        only_w = dev.cloud_records(cloud, qt, D_MIXED, shapes=shapes, per_shape=per_shape, jacobian=False)
        only_j = dev.cloud_records(cloud, qt, D_MIXED, shapes=shapes, per_shape=per_shape, witness=False)
        none = dev.cloud_records(cloud, qt, D_MIXED, shapes=shapes, per_shape=per_shape, witness=False, jacobian=False)
        assert only_w[4] is None and only_j[3] is None and none[3] is None and none[4] is None
        ref = [x.cpu().numpy() for x in both]
        _same(only_w, ref, "witness without rows")
        _same(only_j, ref, "rows without witness")
        _same(none, ref, "neither")
    # null shape / point at the C boundary
    B = qt.shape[0]
    cloud = PointCloud(sets[0], 0.01)
    d = torch.zeros((B,), dtype=torch.float64, device="cuda")
    w = torch.zeros((B, 9), dtype=torch.float64, device="cuda")
    bits = dev._shape_bits(shapes)
    assert lib.nbk_records_cloud_batch(dev._h, cloud._h, qt.data_ptr(), B, D_MIXED, bits.ctypes.data, 0, d.data_ptr(), None, None,
                                       w.data_ptr(), None, dev._stream()) == 0
    torch.cuda.synchronize()
    ref = dev.cloud_records(cloud, q, D_MIXED, shapes=shapes)
    assert_bitwise(d.cpu().numpy(), ref[0], "null shape / point: distance")
    assert_bitwise(w.cpu().numpy(), ref[3], "null shape / point: witness")


@pytest.mark.parametrize("per_shape", [False, True], ids=["per-configuration", "per-shape"])
def test_records_update_and_query_in_one_graph(fresh_world, tmp_path, per_shape, torch_cuda):
    """update + cloud_records captured on one stream with a static points tensor, as test_cloud_update_and_query_in_one_graph has
    it for the clearance: replays see the tensor's current points; the direct call afterwards sees the last cloud."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot("c2m", True, tmp_path)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    sets = [_scan("c2m", N, seed=s) for s in (300, 41, 42)]
    qt = torch.from_numpy(q).cuda()
    Pt = torch.from_numpy(sets[0]).cuda()
    cloud = PointCloud(Pt, 0.01, bounds=([-0.6, -0.6, 0.0], [0.6, 0.6, 1.0]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev.cloud_records(cloud, qt, D_REPLAY, shapes=shapes, per_shape=per_shape)       # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cloud.update(Pt)
            rec = dev.cloud_records(cloud, qt, D_REPLAY, shapes=shapes, per_shape=per_shape)
    torch.cuda.current_stream().wait_stream(side)
    seen = set()
    for k in (1, 2):
        Pt.copy_(torch.from_numpy(sets[k]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in rec]
        raw = Raw(sm, sets[k], 0.01, q, shapes)
        _mixed(cut(raw, D_REPLAY), f"replay {k}")
        _same(got, cut(raw, D_REPLAY, per_shape), f"replay {k}")
        seen.add(got[0].tobytes())
    assert len(seen) == 2, "the clouds must differ"
    _same(dev.cloud_records(cloud, q, D_REPLAY, shapes=shapes, per_shape=per_shape), got, "the eager call after the last replay")
    assert cloud.status() == 0


def test_records_special_inputs(fresh_world, tmp_path, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot("c1", True, tmp_path)
    q = q[:130]
    sm = arm.scene_model()
    nq = sm.kin.n_q
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    S = len(shapes)
    pts = _points("c1")
    cloud = PointCloud(pts, 0.01)

    def filled(got, lead, dist_is, rows_is, what):
        d, s, p, w, j = got
        assert d.shape == lead and w.shape == lead + (9,) and j.shape == lead + (nq,), what
        assert dist_is(d).all() and (s == -1).all() and (p == -1).all() and np.isnan(w).all(), what
        assert rows_is(j), what

    zero_rows = lambda j: np.array_equal(j.view(np.int64), np.zeros(j.shape, dtype=np.int64))        # +0.0, not -0.0
    nan_rows = lambda j: np.isnan(j).all()
    # a NaN joint value in rows 0 and 64: those rows NaN, the others as they were
    qn = q.copy()
    qn[0, 1] = np.nan
    qn[64, nq - 1] = np.nan
    raw = Raw(sm, pts, 0.01, qn, shapes)
    for per_shape in (False, True):
        got = dev.cloud_records(cloud, qn, D_MIXED, shapes=shapes, per_shape=per_shape)
        _same(got, cut(raw, D_MIXED, per_shape), f"NaN rows per_shape={per_shape}")
        lead = (2, S) if per_shape else (2,)
        filled([x[[0, 64]] for x in got], lead, np.isnan, nan_rows, "the NaN rows themselves")
        _same([x[1:64] for x in got], [x[1:64] for x in dev.cloud_records(cloud, q, D_MIXED, shapes=shapes, per_shape=per_shape)], "rows 1..63")
    for per_shape in (False, True):
        lead = (130, S) if per_shape else (130,)
        # a cloud with a non-finite point: its status is set, everything NaN
        bad = pts.copy()
        bad[123, 1] = np.inf
        sick = PointCloud(pts, 0.01)
        sick.update(bad)
        assert sick.status() == 2
        filled(dev.cloud_records(sick, q, D_ALL, shapes=shapes, per_shape=per_shape), lead, np.isnan, nan_rows, "set status")
        # an empty cloud; d_max below every distance: +inf and rows of +0.0
        empty = PointCloud(np.zeros((0, 3)), 0.01, bounds=([-1, -1, 0], [1, 1, 1]), capacity=8)
        filled(dev.cloud_records(empty, q, D_ALL, shapes=shapes, per_shape=per_shape), lead, np.isposinf, zero_rows, "empty cloud")
        filled(dev.cloud_records(cloud, q, -10.0, shapes=shapes, per_shape=per_shape), lead, np.isposinf, zero_rows, "d_max below every distance")
    # an empty selection: +inf per configuration; no column per shape
    filled(dev.cloud_records(cloud, q, D_ALL, shapes=[]), (130,), np.isposinf, zero_rows, "empty selection")
    d, s, p, w, j = dev.cloud_records(cloud, q, D_ALL, shapes=[], per_shape=True)
    assert d.shape == (130, 0) and s.shape == (130, 0) and p.shape == (130, 0) and w.shape == (130, 0, 9) and j.shape == (130, 0, nq)
    assert [x.shape[0] for x in dev.cloud_records(cloud, q[:0], D_ALL, shapes=shapes)] == [0] * 5


def test_records_python_surface(fresh_world, tmp_path, torch_cuda):
    from numbotics_amd.physics import PointCloud, Proximity
    from numbotics_amd.planning import safe_sets
    arm, chain, keep, q = _robot("c1", True, tmp_path)
    q = q[:65]
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    S = sm.n_rshapes
    pts = _points("c1")
    cloud = PointCloud(pts, 0.01)
    base = sm.links[sm.rshape_link[0]]
    shapes = [s for s in range(S) if sm.links[sm.rshape_link[s]]._name != base._name]
    name_of = lambda s: sm.links[sm.rshape_link[s]]._name if s >= 0 else None
    ref = dev.cloud_records(cloud, q, D_MIXED, shapes=shapes)
    near = ref[1] >= 0
    assert near.any() and not near.all()
    d, link, p, w, j = arm.cloud_proximity_jacobians(q, cloud, D_MIXED, ignore_links=[base])
    _same((d, None, p, w, j), ref, "Arm.cloud_proximity_jacobians")
    assert link.shape == (65,) and list(link) == [name_of(s) for s in ref[1]]
    refp = dev.cloud_records(cloud, q, D_MIXED, shapes=shapes, per_shape=True)
    d, link, p, w, j, cols = arm.cloud_proximity_jacobians(q, cloud, D_MIXED, ignore_links=[base._name], per_shape=True)
    _same((d, None, p, w, j), refp, "Arm.cloud_proximity_jacobians per shape")
    assert link.shape == refp[1].shape and list(link.reshape(-1)) == [name_of(s) for s in refp[1].reshape(-1)]
    assert list(cols) == [name_of(s) for s in shapes]
    assert arm.cloud_proximity_jacobians(q.reshape(5, 13, -1), cloud, D_MIXED, ignore_links=[base])[0].shape == (65,)
    # one configuration: a Proximity, or None
    b_near, b_far = int(np.flatnonzero(near)[0]), int(np.flatnonzero(~near)[0])
    prox = arm.cloud_closest_to(q[b_near], cloud, D_MIXED, ignore_links=[base])
    assert isinstance(prox, Proximity) and prox.subject is sm.links[sm.rshape_link[ref[1][b_near]]] and prox.target is cloud
    assert_bitwise(np.concatenate((prox.position_on_subject, prox.position_on_target, prox.normal_target_to_subject)), ref[3][b_near], "Proximity")
    assert_bitwise(np.float64(prox.distance), ref[0][b_near], "Proximity.distance")
    assert arm.cloud_closest_to(q[b_far], cloud, D_MIXED, ignore_links=[base]) is None
    # the IRIS form
    dist, rows = safe_sets.cloud_distance_and_gradient(arm, q, cloud, D_MIXED, ignore_links=[base])
    assert_bitwise(dist, ref[0], "cloud_distance_and_gradient: distance")
    assert_bitwise(rows, ref[4], "cloud_distance_and_gradient: rows")
    last = sm.links[sm.rshape_link[S - 1]]
    of_last = [s for s in range(S) if sm.links[sm.rshape_link[s]]._name == last._name]
    want = dev.cloud_records(cloud, q, D_ALL, shapes=of_last)
    for link_arg in (last, last._name):
        dist, rows = safe_sets.cloud_distance_and_gradient(arm, q, cloud, D_ALL, link=link_arg)
        assert_bitwise(dist, want[0], "one link: distance")
        assert_bitwise(rows, want[4], "one link: rows")
