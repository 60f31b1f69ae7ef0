"""Point-cloud obstacles on the device (nbk_cloud_*, PointCloud, DeviceModel.cloud_validity / cloud_clearance, Arm.in_collision_with_cloud /
cloud_clearance): every mask (bytes and packed words) and every clearance record bit-identical to the CPU oracle run on the same
robot with the cloud's points as sphere world shapes (tests/cloud_cases.py).  Needs a real MI355X.

Every mixed case asserts on the REFERENCE, before comparing, that between 5 % and 70 % of its rows collide, so that no comparison
passes on an all-free or all-colliding mask."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd.scenes import build_scene, sample_q
from test_gpu_parity import assert_bitwise, torch_cuda      # noqa: F401  (fixture)
from cloud_cases import scan, cloud_model, cloud_mask, cloud_closest, pack_bits
import long_chain_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_URDF = os.path.join(ROOT, "tests", "models", "tree_gripper.urdf")
CLOUDS = ((65, 0.02), (300, 0.01), (600, 0.0))        # (N, radius)
THRESHOLDS = (0.0, 0.02, -0.005)
BATCHES = (1, 63, 64, 65, 256)
ROBOTS = [("c1", True), ("c1", False), ("c2m", True), ("c2m", False), ("tree", True), ("tree", False), ("k9", True)]
# the tree gripper is a column 0.25 wide: the scan's wall and table are drawn in to it (x and y scaled, z kept)
SCAN_SCALE = {"tree": np.array([0.4, 0.4, 1.0])}


def _robot(name, margins, tmp):
    """-> (arm, chain, things to keep alive, q (256, dof))."""
    if name == "k9":
        arm, chain, obs = lc.case("k9", tmp)
        return arm, chain, obs, lc.sample(chain, 256, 3)
    if name == "tree":
        from numbotics_amd.physics import GraphChain
        from numbotics_amd.robots import Arm
        chain = GraphChain.from_urdf(TREE_URDF)
        return Arm(chain, bullet_margins=margins), chain, [], sample_q(chain, 256, seed=3)
    arm, chain, obs = build_scene(name, bullet_margins=margins)
    return arm, chain, obs, sample_q(chain, 256, seed=3)


def _scan(name, n, seed=None):
    return np.ascontiguousarray(scan(n, seed=n if seed is None else seed) * SCAN_SCALE.get(name, 1.0))


def _mixed(ref, what):
    f = float(np.mean(ref))
    assert 0.05 <= f <= 0.70, f"{what}: {f:.3f} of the reference collides -- not a mixed case"


def _check_masks(dev, cloud, q, ref, what, shapes=None, thr=0.0, batches=BATCHES):
    for B in batches:
        m = dev.cloud_validity(cloud, q[:B], thr, shapes=shapes)
        assert m.dtype == bool and np.array_equal(m, ref[:B]), f"{what} B={B}: bytes differ at {np.flatnonzero(m != ref[:B])[:8]}"
        w = dev.cloud_validity(cloud, q[:B], thr, packed=True, shapes=shapes)
        assert np.array_equal(w, pack_bits(ref[:B])), f"{what} B={B}: packed words differ"


@pytest.mark.parametrize("name,margins", ROBOTS, ids=[f"{n}-{'bullet' if m else 'sharp'}" for n, m in ROBOTS])
def test_cloud_masks_bitwise(fresh_world, tmp_path, name, margins, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot(name, margins, tmp_path)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    S = sm.n_rshapes
    shapes = list(range(1, S))                                  # the base shape stands on the table
    for N, r in CLOUDS:
        pts = _scan(name, N)
        cloud = PointCloud(pts, r)
        assert cloud.status() == 0 and cloud.n == N
        for thr in THRESHOLDS:
            ref = cloud_mask(sm, pts, r, q, thr, shapes)
            _mixed(ref, f"{name} N={N} r={r} thr={thr}")
            _check_masks(dev, cloud, q, ref, f"{name} N={N} r={r} thr={thr}", shapes, thr)
    # N = 1: the point sits at the frame of the last link that carries a shape, at q[0]
    tool = sm.links[sm.rshape_link[-1]]._name
    p1 = Oracle(sm).fk(q[:1], tool)[0, :3, 3].reshape(1, 3)
    for r, thr in ((0.02, 0.0), (0.01, 0.02), (0.0, 0.02)):
        ref = cloud_mask(sm, p1, r, q, thr, shapes)
        assert ref.any() and not ref.all(), f"{name} N=1: {ref.sum()} of 256 collide"
        _check_masks(dev, PointCloud(p1, r, bounds=([-1, -1, 0], [1, 1, 1])), q, ref, f"{name} N=1 r={r} thr={thr}", shapes, thr)
    # N = 0: nothing collides; and a cloud is empty before its first points
    empty = PointCloud(np.zeros((0, 3)), 0.01, bounds=([-1, -1, 0], [1, 1, 1]), capacity=8)
    _check_masks(dev, empty, q, np.zeros(256, dtype=bool), f"{name} N=0", None, 0.02)


def test_cloud_with_the_base_shape_everything_collides(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    pts = _scan("c1", 65)
    ref = cloud_mask(sm, pts, 0.02, q, 0.02)
    assert ref.all()
    _check_masks(dev, PointCloud(pts, 0.02), q, ref, "every shape", None, 0.02)
    assert arm.in_collision_with_cloud(q, PointCloud(pts, 0.02), 0.02).all()


def test_cloud_grid_edges(fresh_world, torch_cuda):
    """The grid never changes a result: a box that holds half the cloud, cells from a fiftieth of the scene to one cell for all of
    it, coordinates on cell boundaries, 200 points in one cell."""
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    pts = _scan("c1", 300)
    ref = cloud_mask(sm, pts, 0.01, q, 0.0, shapes)
    _mixed(ref, "grid edges")
    lo, hi = pts.min(0), pts.max(0)
    half = (lo, np.array([hi[0], 0.5 * (lo[1] + hi[1]), hi[2]]))      # the y < middle half; the rest is clamped into the border cells
    assert 0.4 < np.mean(np.all(pts <= half[1], axis=1)) < 0.6
    for what, kw in (("half box", dict(bounds=half)), ("cell 0.02", dict(cell=0.02)), ("cell 0.1", dict(cell=0.1)),
                     ("one cell", dict(cell=10.0)), ("half box, cell 0.02", dict(bounds=half, cell=0.02)),
                     ("box elsewhere", dict(bounds=([5, 5, 5], [6, 6, 6]), cell=0.1))):
        cloud = PointCloud(pts, 0.01, **kw)
        if what == "one cell":
            assert tuple(cloud.dims) == (1, 1, 1)
        _check_masks(dev, cloud, q, ref, what, shapes, 0.0, batches=(65, 256))
    # coordinates that are exact multiples of the cell (a power of two: the products are exact), lo at a multiple too
    cell = 0.0625
    snapped = np.round(pts / cell) * cell
    ref_s = cloud_mask(sm, snapped, 0.01, q, 0.0, shapes)
    _mixed(ref_s, "snapped")
    for lo_s in ([-1.0, -1.0, 0.0], [0.0, 0.0, 0.0]):
        _check_masks(dev, PointCloud(snapped, 0.01, cell=cell, bounds=(lo_s, [1.0, 1.0, 1.0])), q, ref_s, f"snapped lo={lo_s}", shapes, 0.0, batches=(256,))
    # 200 points in a single cell, the rest of the scan around them
    rng = np.random.default_rng(5)
    crowd = np.array([0.45, 0.0, 0.5]) + rng.uniform(0.001, 0.009, (200, 3))
    both = np.concatenate((pts[:100], crowd))
    ref_c = cloud_mask(sm, both, 0.01, q, 0.0, shapes)
    _mixed(ref_c, "crowded cell")
    cloud = PointCloud(both, 0.01, cell=0.1, bounds=([-1.0, -1.0, 0.0], [1.0, 1.0, 1.0]))
    from numbotics_amd.physics.pointcloud import cells_host
    assert len(np.unique(cells_host(cloud.lo, cloud.cell, cloud.dims, crowd))) == 1
    _check_masks(dev, cloud, q, ref_c, "crowded cell", shapes, 0.0, batches=(256,))


def test_cloud_reuse(fresh_world, torch_cuda):
    """One object updated 600 -> 65 -> 600 (other points) -> 0 points equals a fresh object each time; more than the capacity is refused."""
    from numbotics_amd.physics import PointCloud
    from numbotics_amd._lib import NbkError
    arm, chain, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    first = _scan("c1", 600)
    cloud = PointCloud(first, 0.01, capacity=600)
    box = ([-0.6, -0.6, 0.0], [0.6, 0.6, 1.0])
    for k, (pts, r) in enumerate(((first, 0.01), (_scan("c1", 65), 0.02), (_scan("c1", 600, seed=77), 0.0), (np.zeros((0, 3)), 0.0), (first, 0.01))):
        if k > 0:
            cloud.update(pts, radius=r)
        ref = cloud_mask(sm, pts, r, q, 0.0, shapes)
        if pts.shape[0] > 0:
            _mixed(ref, f"reuse step {k}")
        m = dev.cloud_validity(cloud, q, 0.0, shapes=shapes)
        fresh = dev.cloud_validity(PointCloud(pts, r, bounds=box), q, 0.0, shapes=shapes)
        assert np.array_equal(m, ref) and np.array_equal(fresh, ref), f"reuse step {k}"
        d, s, p = dev.cloud_clearance(cloud, q, 0.05, shapes=shapes)
        dr, sr, pr = cloud_closest(sm, pts, r, q, 0.05, shapes)
        assert_bitwise(d, dr, f"reuse step {k}: clearance")
        assert np.array_equal(s, sr) and np.array_equal(p, pr)
    with pytest.raises(NbkError, match="NBK_ERR_INVALID"):
        cloud.update(_scan("c1", 601), radius=0.5)
    assert cloud.radius == 0.01 and cloud.n == 600, "a refused update leaves the object's own record as the device has it"
    assert np.array_equal(dev.cloud_validity(cloud, q, 0.0, shapes=shapes), ref), "a refused update changes nothing"


def test_cloud_shape_selection(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    S = sm.n_rshapes
    pts = _scan("c1", 300)
    cloud = PointCloud(pts, 0.01)
    seen = []
    for shapes in ([S - 1], [3, 5], list(range(4, S)), list(range(1, S, 2)), [2, 1]):
        ref = cloud_mask(sm, pts, 0.01, q, 0.02, shapes)
        seen.append(ref.mean())
        _check_masks(dev, cloud, q, ref, f"shapes {shapes}", shapes, 0.02, batches=(65, 256))
    assert max(seen) >= 0.05 and len(set(seen)) > 2, seen       # the selections matter
    _check_masks(dev, cloud, q, np.zeros(256, dtype=bool), "empty selection", [], 0.02, batches=(256,))
    d, s, p = dev.cloud_clearance(cloud, q, 0.5, shapes=[])
    assert np.all(np.isposinf(d)) and np.all(s == -1) and np.all(p == -1)
    # ignore_links: the links' shapes are left out
    base = sm.links[sm.rshape_link[0]]
    last = sm.links[sm.rshape_link[S - 1]]
    for ignore in ([base], [base._name, last._name]):
        names = {getattr(l, "_name", l) for l in ignore}
        shapes = [s_ for s_ in range(S) if sm.links[sm.rshape_link[s_]]._name not in names]
        ref = cloud_mask(sm, pts, 0.01, q, 0.0, shapes)
        _mixed(ref, f"ignore {names}")
        got = arm.in_collision_with_cloud(q, cloud, ignore_links=ignore)
        assert np.array_equal(got, ref)
        assert arm.in_collision_with_cloud(q.reshape(4, 64, -1), cloud, ignore_links=ignore).shape == (4, 64)
        b = int(np.flatnonzero(ref)[0]), int(np.flatnonzero(~ref)[0])
        assert arm.in_collision_with_cloud(q[b[0]], cloud, ignore_links=ignore) is True
        assert arm.in_collision_with_cloud(q[b[1]], cloud, ignore_links=ignore) is False
        dr, sr, pr = cloud_closest(sm, pts, 0.01, q, 0.05, shapes)
        d, link, p = arm.cloud_clearance(q, cloud, 0.05, ignore_links=ignore)
        assert_bitwise(d, dr, "Arm.cloud_clearance")
        assert np.array_equal(p, pr)
        assert list(link) == [sm.links[sm.rshape_link[s_]]._name if s_ >= 0 else None for s_ in sr]
    with pytest.raises(ValueError):
        arm.in_collision_with_cloud(q, cloud, ignore_links=["no_such_link"])


def test_cloud_accumulate(fresh_world, torch_cuda):
    """validity of c2 (its cube), then the cloud's verdicts ORed into the same mask = the oracle's mask of the combined model."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot("c2", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    pts = _scan("c2", 300)
    cloud = PointCloud(pts, 0.01)
    own = Oracle(sm).validity(q, 0.0)
    only = cloud_mask(sm, pts, 0.01, q, 0.0, shapes)
    ref = Oracle(cloud_model(sm, pts, 0.01, shapes, keep_scene=True)).validity(q, 0.0)
    assert np.array_equal(ref, own | only)
    _mixed(ref, "combined")
    assert (own & ~only).any() and (only & ~own).any(), "each side must add rows of its own"
    qt = torch.from_numpy(q).cuda()
    for B in BATCHES:
        mask = dev.validity(qt[:B], 0.0)                                    # bool tensor
        assert np.array_equal(mask.cpu().numpy(), own[:B])
        got = dev.cloud_validity(cloud, qt[:B], 0.0, shapes=shapes, out=mask)
        assert got is mask and np.array_equal(mask.cpu().numpy(), ref[:B]), f"bytes B={B}"
        words = dev.validity(qt[:B], 0.0, packed=True)
        guard = words.clone()
        dev.cloud_validity(cloud, qt[:B], 0.0, packed=True, shapes=shapes, out=words)
        assert np.array_equal(words.cpu().numpy(), pack_bits(ref[:B])), f"words B={B}"
        # bits beyond B: left alone when accumulating, written 0 when overwriting
        if B % 64:
            high = torch.full_like(guard, -1)
            dev.cloud_validity(cloud, qt[:B], 0.0, packed=True, shapes=shapes, out=high)
            tail = np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(B % 64)
            assert (high.cpu().numpy().view(np.uint64)[-1] & tail) == tail
            over = dev.cloud_validity(cloud, qt[:B], 0.0, packed=True, shapes=shapes)
            assert (over.cpu().numpy().view(np.uint64)[-1] & tail) == 0
        # a cleared mask and accumulate = overwrite
        zero = torch.zeros((B,), dtype=torch.uint8, device="cuda")
        dev.cloud_validity(cloud, qt[:B], 0.0, shapes=shapes, out=zero)
        assert np.array_equal(zero.cpu().numpy().astype(bool), only[:B])
    for bad in (own, [0] * 256, mask[:5], mask.float(), mask.cpu()):       # not a tensor; wrong shape, dtype, device
        with pytest.raises(ValueError, match="out must be"):
            dev.cloud_validity(cloud, qt, 0.0, shapes=shapes, out=bad)


@pytest.mark.parametrize("name", ["c1", "c2m"])
def test_cloud_clearance_bitwise(fresh_world, name, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot(name, True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    S = sm.n_rshapes
    shapes = list(range(1, S))
    pts = _scan(name, 600)
    pts[599] = pts[7]; pts[300] = pts[450]                      # duplicated points: ties go to the smaller index
    dist = Oracle(cloud_model(sm, pts, 0.0, shapes)).pair_distances(q)
    assert_bitwise(dist.min(1), Oracle(cloud_model(sm, pts, 0.0, shapes)).closest(q)[0], "the oracle's closest is the first minimum")
    for r in (0.0, 0.01):
        cloud = PointCloud(pts, r)
        for d_max in (0.02, 0.5):
            dr, sr, pr = cloud_closest(sm, pts, r, q, d_max, shapes)
            fin = np.isfinite(dr)
            if d_max == 0.02:
                assert 0.10 <= fin.mean() <= 0.90, fin.mean()
            assert (dr[fin] < 0).any(), "no penetrating rows in the reference"
            for B in (65, 256):
                d, s, p = dev.cloud_clearance(cloud, q[:B], d_max, shapes=shapes)
                assert_bitwise(d, dr[:B], f"{name} r={r} d_max={d_max} B={B}: distance")
                assert np.array_equal(s, sr[:B]), f"{name} r={r} d_max={d_max}: shape"
                assert np.array_equal(p, pr[:B]), f"{name} r={r} d_max={d_max}: point"
                assert np.array_equal(np.isposinf(d), ~fin[:B])
    assert not np.any(pr == 599) and not np.any(pr == 450)
    # every shape: the base stands in the table's points
    dr, sr, pr = cloud_closest(sm, pts, 0.0, q, 0.5)
    d, s, p = dev.cloud_clearance(PointCloud(pts, 0.0), q, 0.5)
    assert_bitwise(d, dr, "every shape")
    assert np.array_equal(s, sr) and np.array_equal(p, pr)


def test_cloud_non_finite(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    pts = _scan("c1", 300)
    ref = cloud_mask(sm, pts, 0.01, q, 0.0, shapes)
    dr, sr, pr = cloud_closest(sm, pts, 0.01, q, 0.05, shapes)
    cloud = PointCloud(pts, 0.01)
    for bad_value in (np.nan, np.inf):
        bad = pts.copy()
        bad[123, 1] = bad_value
        cloud.update(bad)
        assert cloud.status() == 2
        assert dev.cloud_validity(cloud, q, 0.0, shapes=shapes).all()
        assert np.array_equal(dev.cloud_validity(cloud, q[:65], 0.0, packed=True, shapes=shapes), pack_bits(np.ones(65, dtype=bool)))
        d, s, p = dev.cloud_clearance(cloud, q, 0.05, shapes=shapes)
        assert np.all(np.isnan(d)) and np.all(s == -1) and np.all(p == -1)
        cloud.update(pts)
        assert cloud.status() == 0
        assert np.array_equal(dev.cloud_validity(cloud, q, 0.0, shapes=shapes), ref)
        d, s, p = dev.cloud_clearance(cloud, q, 0.05, shapes=shapes)
        assert_bitwise(d, dr, "after a clean update")
        assert np.array_equal(s, sr) and np.array_equal(p, pr)
    # a non-finite q row collides, and only that row
    for bad_value in (np.nan, -np.inf):
        qn = q.copy()
        free = int(np.flatnonzero(~ref)[3])
        qn[free, 2] = bad_value
        want = ref.copy()
        want[free] = True
        assert np.array_equal(dev.cloud_validity(cloud, qn, 0.0, shapes=shapes), want)
        assert np.array_equal(dev.cloud_validity(cloud, qn, 0.0, packed=True, shapes=shapes), pack_bits(want))
        d, s, p = dev.cloud_clearance(cloud, qn, 0.05, shapes=shapes)
        assert np.isnan(d[free]) and s[free] == -1 and p[free] == -1
        keep_rows = np.arange(256) != free
        assert_bitwise(d[keep_rows], dr[keep_rows], "the other rows")


def test_cloud_update_and_query_in_one_graph(fresh_world, torch_cuda):
    """update + cloud_validity + cloud_clearance captured on one stream with a static points tensor; replays see the tensor's
    current points; a direct call afterwards sees the last cloud."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    shapes = list(range(1, sm.n_rshapes))
    sets = [_scan("c1", 300, seed=s) for s in (300, 41, 42, 43)]
    qt = torch.from_numpy(q).cuda()
    Pt = torch.from_numpy(sets[0]).cuda()
    cloud = PointCloud(Pt, 0.01, bounds=([-0.6, -0.6, 0.0], [0.6, 0.6, 1.0]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev.cloud_validity(cloud, qt, 0.0, shapes=shapes)                   # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cloud.update(Pt)
            mask = dev.cloud_validity(cloud, qt, 0.0, shapes=shapes)
            d, s, p = dev.cloud_clearance(cloud, qt, 0.05, shapes=shapes)
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 2, 3):
        Pt.copy_(torch.from_numpy(sets[k]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        ref = cloud_mask(sm, sets[k], 0.01, q, 0.0, shapes)
        _mixed(ref, f"replay {k}")
        assert np.array_equal(mask.cpu().numpy(), ref), f"replay {k}"
        dr, sr, pr = cloud_closest(sm, sets[k], 0.01, q, 0.05, shapes)
        assert_bitwise(d.cpu().numpy(), dr, f"replay {k}: clearance")
        assert np.array_equal(s.cpu().numpy(), sr) and np.array_equal(p.cpu().numpy(), pr)
    assert len({cloud_mask(sm, sets[k], 0.01, q, 0.0, shapes).tobytes() for k in (1, 2, 3)}) == 3, "the three clouds must differ"
    assert np.array_equal(dev.cloud_validity(cloud, q, 0.0, shapes=shapes), ref), "a direct call sees the last cloud"
    assert cloud.status() == 0


def test_cloud_c_boundary(fresh_world, torch_cuda):
    """Argument errors at the C boundary; null optional outputs; calls on a capturing stream allocate nothing and leave the capture
    usable.

    The wrong-device case needs a second GPU: with one visible device that block does not run, and the device check of the cloud
    entries (cloud_check_device) is then not exercised by this suite."""
    torch = torch_cuda
    from numbotics_amd import _lib
    from numbotics_amd.physics import PointCloud
    lib = _lib.load()
    arm, chain, keep, q = _robot("c1", True, None)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    pts = _scan("c1", 300)
    ref = cloud_mask(sm, pts, 0.01, q, 0.0)
    dr, sr, pr = cloud_closest(sm, pts, 0.01, q, 0.05)
    cloud = PointCloud(pts, 0.01, capacity=400)
    qt = torch.from_numpy(q).cuda()
    pt = torch.from_numpy(pts).cuda()
    B = 256
    bytes_ = torch.zeros((B,), dtype=torch.uint8, device="cuda")
    words = torch.zeros((4,), dtype=torch.int64, device="cuda")
    d = torch.zeros((B,), dtype=torch.float64, device="cuda")
    INVALID = -1
    val, clr, setp = lib.nbk_cloud_validity_batch, lib.nbk_cloud_clearance_batch, lib.nbk_cloud_set_points
    # both masks at once; only one; none
    assert val(dev._h, cloud._h, qt.data_ptr(), B, 0.0, None, 0, words.data_ptr(), bytes_.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bytes_.cpu().numpy().astype(bool), ref) and np.array_equal(words.cpu().numpy(), pack_bits(ref))
    assert val(dev._h, cloud._h, qt.data_ptr(), B, 0.0, None, 0, None, None, None) == INVALID
    assert val(dev._h, cloud._h, None, B, 0.0, None, 0, words.data_ptr(), None, None) == INVALID
    assert val(dev._h, None, qt.data_ptr(), B, 0.0, None, 0, words.data_ptr(), None, None) == INVALID
    assert val(None, cloud._h, qt.data_ptr(), B, 0.0, None, 0, words.data_ptr(), None, None) == INVALID
    assert val(dev._h, cloud._h, qt.data_ptr(), -1, 0.0, None, 0, words.data_ptr(), None, None) == INVALID
    assert val(dev._h, cloud._h, None, 0, 0.0, None, 0, None, None, None) == 0                       # B = 0: nothing to do
    # clearance: optional shape / point outputs; d_max must be finite
    assert clr(dev._h, cloud._h, qt.data_ptr(), B, 0.05, None, d.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    assert_bitwise(d.cpu().numpy(), dr, "distance alone")
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert clr(dev._h, cloud._h, qt.data_ptr(), B, bad, None, d.data_ptr(), None, None, None) == INVALID
    assert clr(dev._h, cloud._h, qt.data_ptr(), B, 0.05, None, None, None, None, None) == INVALID
    # updates
    assert setp(cloud._h, pt.data_ptr(), 401, 0.01, None) == INVALID
    assert setp(cloud._h, pt.data_ptr(), -1, 0.01, None) == INVALID
    assert setp(cloud._h, None, 3, 0.01, None) == INVALID
    assert setp(cloud._h, pt.data_ptr(), 300, float("nan"), None) == INVALID
    assert setp(cloud._h, pt.data_ptr(), 300, -0.01, None) == INVALID
    assert np.array_equal(dev.cloud_validity(cloud, q, 0.0), ref), "refused updates change nothing"
    # another device current: refused (where there is one)
    if torch.cuda.device_count() >= 2:
        with torch.cuda.device(1):
            assert val(dev._h, cloud._h, qt.data_ptr(), B, 0.0, None, 0, words.data_ptr(), None, None) == INVALID
            assert setp(cloud._h, pt.data_ptr(), 300, 0.01, None) == INVALID
            st = C.c_int32(0)
            assert lib.nbk_cloud_status(cloud._h, C.byref(st)) == INVALID
    # a capturing stream: every call is a graph node, nothing allocates or synchronises (either would end the capture with an error)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st = C.c_void_p(side.cuda_stream)
        g = torch.cuda.CUDAGraph()
        g.capture_begin()
        assert setp(cloud._h, pt.data_ptr(), 300, 0.01, st) == 0
        assert val(dev._h, cloud._h, qt.data_ptr(), B, 0.0, None, 0, words.data_ptr(), bytes_.data_ptr(), st) == 0
        assert clr(dev._h, cloud._h, qt.data_ptr(), B, 0.05, None, d.data_ptr(), None, None, st) == 0
        assert val(dev._h, cloud._h, qt.data_ptr(), B, 0.0, None, 0, None, None, st) == INVALID        # refused without breaking the capture
        g.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    bytes_.zero_(); words.zero_(); d.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bytes_.cpu().numpy().astype(bool), ref) and np.array_equal(words.cpu().numpy(), pack_bits(ref))
    assert_bitwise(d.cpu().numpy(), dr, "replayed clearance")
