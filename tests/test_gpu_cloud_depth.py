"""Depth frames to point clouds on the device (nbk_frame_cloud_backproject, nbk_frame_cloud_self_filter, nbk_frame_cloud_set_points; backproject,
Arm.cloud_self_filter, PointCloud.update(keep=) / count / update_from_depth): the back-projection bit for bit its NumPy restatement,
the self-filter bit for bit the CPU oracle's verdict per point, the masked update equal to a cloud of the kept points, and the three
together -- eagerly and in a replayed graph.  Needs a real MI355X.

Every self-filter case asserts on the REFERENCE, before comparing, that it removes between 5 % and 70 % of the points (the same
condition runs without a device in tests/test_cloud_depth_host.py); the mask comparisons assert that their reference is mixed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from numbotics_amd.scenes import sample_q
from test_gpu_parity import assert_bitwise, torch_cuda      # noqa: F401  (fixture)
from cloud_cases import scan, cloud_mask, cloud_closest
import cloud_depth_cases as dc
import cloud_fuse_cases as fc
import long_chain_cases as lc

CUTS = (1, 63, 64, 65, 255, 256, 257)


def _mixed(ref, what):
    f = float(np.mean(ref))
    assert 0.05 <= f <= 0.70, f"{what}: {f:.3f} of the reference collides -- not a mixed case"


def _rows(name, chain):
    return lc.sample(chain, 256, 3) if name == "k9" else sample_q(chain, 256, seed=3)


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{what}: bits differ"


# ---- 1. back-projection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_backproject_bitwise(torch_cuda, kind):
    torch = torch_cuda
    from numbotics_amd.physics import backproject
    scale = 1.0 if kind == "f32" else 0.001
    T = dc.camera_pose()
    for H, W in dc.SHAPES:
        d = dc.depth_image(H, W, kind)
        intr = dc.intrinsics(H, W)
        rp, rk = dc.backproject_ref(d, intr, T, scale, dc.Z_MIN, dc.Z_MAX)
        pts, keep = backproject(d, intr, T, depth_scale=scale, z_min=dc.Z_MIN, z_max=dc.Z_MAX)
        assert pts.is_cuda and keep.is_cuda and pts.dtype == torch.float64 and keep.dtype == torch.uint8
        _bits(keep.cpu().numpy(), rk, f"{W}x{H} {kind}: keep")
        _bits(pts.cpu().numpy(), rp, f"{W}x{H} {kind}: points")
        # a CUDA image (a torch 16-bit tensor is read as unsigned raw bits), out=, and the pose rewritten on the device between two calls
        dt = torch.from_numpy(d.view(np.int16) if kind == "u16" else d).cuda()
        Tt = torch.from_numpy(np.ascontiguousarray(T)).cuda()
        out = (torch.full((H * W, 3), -1.0, dtype=torch.float64, device="cuda"), torch.full((H * W,), 7, dtype=torch.uint8, device="cuda"))
        got = backproject(dt, intr, Tt, depth_scale=scale, z_min=dc.Z_MIN, z_max=dc.Z_MAX, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        _bits(out[0].cpu().numpy(), rp, f"{W}x{H} {kind}: points (device image)")
        _bits(out[1].cpu().numpy(), rk, f"{W}x{H} {kind}: keep (device image)")
        T2 = T.copy()
        T2[:3, :3] = T[:3, :3].T
        T2[:3, 3] = [-0.5, 0.25, 1.5]
        Tt.copy_(torch.from_numpy(T2).cuda())
        backproject(dt, intr, Tt, depth_scale=scale, z_min=dc.Z_MIN, z_max=dc.Z_MAX, out=out)
        rp2, rk2 = dc.backproject_ref(d, intr, T2, scale, dc.Z_MIN, dc.Z_MAX)
        _bits(out[0].cpu().numpy(), rp2, f"{W}x{H} {kind}: points (pose rewritten)")
        _bits(out[1].cpu().numpy(), rk2, f"{W}x{H} {kind}: keep (pose rewritten)")
        if H * W > 8:
            assert not np.array_equal(rp, rp2)
    # the reference's camera frame, as a host pose and as a device pose
    d = dc.depth_image(17, 33, kind)
    intr = dc.intrinsics(17, 33)
    from numbotics_amd.physics.pointcloud import optical_pose
    rp, rk = dc.backproject_ref(d, intr, optical_pose(T, "numbotics"), scale, dc.Z_MIN, dc.Z_MAX)
    for pose in (T, torch.from_numpy(np.ascontiguousarray(T)).cuda()):
        pts, keep = backproject(d, intr, pose, depth_scale=scale, z_min=dc.Z_MIN, z_max=dc.Z_MAX, frame="numbotics")
        _bits(pts.cpu().numpy(), rp, "numbotics frame: points")
        _bits(keep.cpu().numpy(), rk, "numbotics frame: keep")


# ---- 2. self-filter, 4. seam -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,margins", dc.ROBOTS, ids=dc.ROBOT_IDS)
def test_self_filter_bitwise(fresh_world, tmp_path, name, margins, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, alive, q0 = dc.robot(name, margins, tmp_path)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    S = sm.n_rshapes
    pts = dc.frame_points(name, sm, q0)
    N = pts.shape[0]
    for r, pad in dc.FILTER_PARAMS:
        ref = dc.filter_ref(sm, pts, r, q0, pad)
        dc.in_band(ref, f"{name} r={r} pad={pad}")
        for n in CUTS + (N,):
            if n > N:
                continue
            got = dev.cloud_self_filter(pts[:n], q0, r, pad)
            assert got.dtype == bool and got.shape == (n,)
            assert np.array_equal(got, ref[:n]), f"{name} r={r} pad={pad} N={n}: differs at {np.flatnonzero(got != ref[:n])[:8]}"
        # the seam: a cloud of the points kept reads free at (q0, padding) -- the same predicate
        cloud = PointCloud(pts, r)
        cloud.update(pts, keep=ref)
        assert cloud.count() == int(ref.sum()) and cloud.status() == 0
        assert not dev.cloud_validity(cloud, q0.reshape(1, -1), pad)[0], f"{name} r={r} pad={pad}: the filtered cloud collides at q0"
        if pad == 0.02:
            cloud.update(pts)
            assert dev.cloud_validity(cloud, q0.reshape(1, -1), pad)[0], "the unfiltered cloud collides at q0"
    r, pad = dc.FILTER_PARAMS[0]
    ref = dc.filter_ref(sm, pts, r, q0, pad)
    # the set has fewer than 256 points on most robots: twice the set (the copy shifted by a millimetre) reaches the cuts around one
    # workgroup's 256 points and a grid of two workgroups
    two = np.ascontiguousarray(np.concatenate((pts, pts[::-1] + 1e-3)))
    ref_two = dc.filter_ref(sm, two, r, q0, pad)
    dc.in_band(ref_two, f"{name}: twice the set")
    assert two.shape[0] > 257
    for n in (255, 256, 257, two.shape[0]):
        got = dev.cloud_self_filter(two[:n], q0, r, pad)
        assert np.array_equal(got, ref_two[:n]), f"{name} twice the set N={n}: differs at {np.flatnonzero(got != ref_two[:n])[:8]}"
    # a keep that comes in with zeros: they stay zero, the others are decided as before; the tensor is worked on in place
    rng = np.random.default_rng(3)
    k0 = rng.uniform(size=N) < 0.5
    kt = torch.from_numpy(k0.astype(np.uint8)).cuda()
    pt = torch.from_numpy(pts).cuda()
    assert dev.cloud_self_filter(pt, torch.from_numpy(q0).cuda(), r, pad, keep=kt) is kt
    assert np.array_equal(kt.cpu().numpy().astype(bool), k0 & ref)
    assert (k0 & ~ref).any() and (~k0 & ~ref).any()
    # a selection of shapes, and of links through the arm
    sel = list(range(1, S, 2))
    ref_sel = dc.filter_ref(sm, pts, r, q0, pad, sel)
    assert ref_sel.sum() > ref.sum() and not ref_sel.all(), "the selection matters"
    assert np.array_equal(dev.cloud_self_filter(pts, q0, r, pad, shapes=sel), ref_sel)
    assert dev.cloud_self_filter(pts, q0, r, pad, shapes=[]).all(), "an empty selection removes nothing"
    base = sm.links[sm.rshape_link[0]]
    rest = [s for s in range(S) if sm.links[sm.rshape_link[s]]._name != base._name]
    ref_rest = dc.filter_ref(sm, pts, r, q0, pad, rest)
    assert np.array_equal(arm.cloud_self_filter(pts, q0, r, pad, ignore_links=[base]), ref_rest)
    only = [s for s in range(S) if s not in rest]
    assert np.array_equal(arm.cloud_self_filter(pts, q0, r, pad, links=[base._name]), dc.filter_ref(sm, pts, r, q0, pad, only))
    # N = 0; a non-finite q0 removes nothing
    assert dev.cloud_self_filter(np.zeros((0, 3)), q0, r, pad).shape == (0,)
    for bad in (np.nan, np.inf):
        qb = q0.copy()
        qb[-1] = bad
        assert dev.cloud_self_filter(pts, qb, r, pad).all(), f"q0 with {bad}"


# ---- 3. masked update ---------------------------------------------------------------------------------------------------------------
def test_masked_update_is_the_cloud_of_the_kept_points(fresh_world, tmp_path, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, alive, q0 = dc.robot("c1", True, tmp_path)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    q = _rows("c1", chain)
    shapes = list(range(1, sm.n_rshapes))
    pts = np.ascontiguousarray(scan(300, seed=300))            # (the wall and the table: the masks of the 256 rows are mixed)
    N = pts.shape[0]
    r = 0.01
    box = ([-0.7, -0.7, 0.0], [0.7, 0.7, 1.3])
    cloud = PointCloud(pts, r, bounds=box)
    assert cloud.count() == N
    for seed, frac in ((1, 0.6), (2, 0.2), (3, 0.95)):
        k = np.random.default_rng(seed).uniform(size=N) < frac
        orig = np.flatnonzero(k)
        cloud.update(pts, keep=k)
        compact = PointCloud(pts[k], r, bounds=box)
        assert cloud.count() == orig.shape[0] == compact.count() and cloud.n == N and cloud.status() == 0
        for thr in (0.0, 0.02):
            ref = cloud_mask(sm, pts[k], r, q, thr, shapes)
            _mixed(ref, f"masked update seed {seed} thr {thr}")
            a = dev.cloud_validity(cloud, q, thr, shapes=shapes)
            b = dev.cloud_validity(compact, q, thr, shapes=shapes)
            assert np.array_equal(a, b) and np.array_equal(a, ref), f"seed {seed} thr {thr}"
            assert np.array_equal(dev.cloud_validity(cloud, q, thr, packed=True, shapes=shapes),
                                  dev.cloud_validity(compact, q, thr, packed=True, shapes=shapes))
        d, s, p = dev.cloud_clearance(cloud, q, 0.05, shapes=shapes)
        dcmp, scmp, pcmp = dev.cloud_clearance(compact, q, 0.05, shapes=shapes)
        dr, sr, pr = cloud_closest(sm, pts[k], r, q, 0.05, shapes)
        assert_bitwise(d, dcmp, f"seed {seed}: clearance")
        assert_bitwise(d, dr, f"seed {seed}: clearance against the oracle")
        assert np.array_equal(s, scmp) and np.array_equal(s, sr)
        near = pcmp >= 0
        assert near.any() and not near.all()
        assert np.array_equal(p[near], orig[pcmp[near]]) and np.all(p[~near] == -1), "point is the ORIGINAL index"
    # a device mask (uint8 and bool), read in place
    k = np.random.default_rng(1).uniform(size=N) < 0.6
    ref = cloud_mask(sm, pts[k], r, q, 0.0, shapes)
    for kt in (torch.from_numpy(k.astype(np.uint8)).cuda(), torch.from_numpy(k).cuda()):
        cloud.update(torch.from_numpy(pts).cuda(), keep=kt)
        assert np.array_equal(dev.cloud_validity(cloud, q, 0.0, shapes=shapes), ref) and cloud.count() == int(k.sum())
    # nothing kept: the empty cloud
    cloud.update(pts, keep=np.zeros(N, dtype=bool))
    assert cloud.count() == 0 and cloud.status() == 0
    assert not dev.cloud_validity(cloud, q, 0.05, shapes=shapes).any()
    d, s, p = dev.cloud_clearance(cloud, q, 0.5, shapes=shapes)
    assert np.all(np.isposinf(d)) and np.all(s == -1) and np.all(p == -1)
    # a NaN point masked out is not looked at; kept, it sets the status
    bad = pts.copy()
    bad[5] = [np.nan, 0.0, np.inf]
    k = np.ones(N, dtype=bool)
    k[5] = False
    cloud.update(bad, keep=k)
    assert cloud.status() == 0 and cloud.count() == N - 1
    assert np.array_equal(dev.cloud_validity(cloud, q, 0.0, shapes=shapes), cloud_mask(sm, pts[k], r, q, 0.0, shapes))
    cloud.update(bad, keep=np.ones(N, dtype=bool))
    assert cloud.status() == 2 and dev.cloud_validity(cloud, q, 0.0, shapes=shapes).all()
    cloud.update(pts)
    assert cloud.status() == 0 and cloud.count() == N, "the plain update is the same call without a mask"
    with pytest.raises(ValueError):
        cloud.update(pts, keep=np.ones(N - 1, dtype=bool))


# ---- 5. pipeline, 6. graph ---------------------------------------------------------------------------------------------------------
H, W = 17, 33
CAM = np.array([[1.0, 0.0, 0.0, -1.6], [0.0, 1.0, 0.0, 0.05], [0.0, 0.0, 1.0, 0.55], [0.0, 0.0, 0.0, 1.0]])      # looks along world x, z up
RADIUS, PAD = 0.01, 0.02


def _frame(name, sm, q0, cam=CAM):
    """(depth (H, W) float32, intrinsics): the case's points seen by the 33x17 camera."""
    from numbotics_amd.physics import intrinsics_from_fov
    from numbotics_amd.physics.pointcloud import optical_pose
    intr = intrinsics_from_fov(W, H, 50.0)
    To = np.concatenate((optical_pose(cam, "numbotics"), [[0.0, 0.0, 0.0, 1.0]]))
    return dc.project_points(dc.frame_points(name, sm, q0), To, intr, H, W), intr


def _pipeline_ref(sm, depth, intr, cam, q0, shapes):
    """restatement -> filter_ref -> (points, keep): what update_from_depth must leave in the cloud."""
    from numbotics_amd.physics.pointcloud import optical_pose
    pts, keep = dc.backproject_ref(depth, intr, optical_pose(cam, "numbotics"))
    keep = keep.astype(bool)
    idx = np.flatnonzero(keep)
    keep[idx] = dc.filter_ref(sm, pts[idx], RADIUS, q0, PAD, shapes)
    return pts, keep, idx.shape[0]


def test_update_from_depth_pipeline(fresh_world, tmp_path, torch_cuda):
    from numbotics_amd.physics import PointCloud
    arm, chain, alive, q0 = dc.robot("c1", True, tmp_path)
    sm = arm.scene_model()
    q = _rows("c1", chain)
    base = sm.links[sm.rshape_link[0]]
    shapes = [s for s in range(sm.n_rshapes) if sm.links[sm.rshape_link[s]]._name != base._name]
    depth, intr = _frame("c1", sm, q0)
    pts, keep, n_valid = _pipeline_ref(sm, depth, intr, CAM, q0, shapes)
    removed = 1.0 - keep.sum() / n_valid
    assert n_valid > 64 and 0.05 <= removed <= 0.70, f"{n_valid} pixels, the filter removes {removed:.3f}"
    cloud = PointCloud(np.zeros((0, 3)), RADIUS, bounds=([-0.7, -0.7, 0.0], [0.7, 0.7, 1.3]), capacity=H * W)
    for dep in (depth, depth.copy()):                           # the second call reuses the staging of the first
        gp, gk = cloud.update_from_depth(dep, intr, CAM, arm=arm, q=q0, padding=PAD, ignore_links=[base], frame="numbotics")
        _bits(gk.cpu().numpy().astype(bool), keep, "pipeline: keep")
        _bits(gp.cpu().numpy(), pts, "pipeline: points")
        assert cloud.count() == int(keep.sum()) and cloud.status() == 0
        ref = cloud_mask(sm, pts[keep], RADIUS, q, PAD, shapes)
        _mixed(ref, "pipeline")
        got = arm.in_collision_with_cloud(q, cloud, PAD, ignore_links=[base])
        assert np.array_equal(got, ref), f"pipeline: masks differ at {np.flatnonzero(got != ref)[:8]}"
        assert not arm.in_collision_with_cloud(q0, cloud, PAD, ignore_links=[base])
    # a clearance record's point is a pixel
    d, names, p = arm.cloud_clearance(q, cloud, 0.05, ignore_links=[base])
    assert (p >= 0).any() and keep[p[p >= 0]].all() and (depth.reshape(-1)[p[p >= 0]] > 0).all()
    # without the arm nothing is filtered: the frame's own image of the arm collides at q0
    cloud.update_from_depth(depth, intr, CAM, frame="numbotics")
    assert cloud.count() == n_valid and arm.in_collision_with_cloud(q0, cloud, PAD, ignore_links=[base])
    # 16-bit frames go the same way
    from numbotics_amd.physics.pointcloud import optical_pose
    mm = np.round(depth.astype(np.float64) * 1000.0).astype(np.uint16)
    pts16, keep16 = dc.backproject_ref(mm, intr, optical_pose(CAM, "numbotics"), 0.001)
    gp, gk = cloud.update_from_depth(mm, intr, CAM, frame="numbotics", depth_scale=0.001)
    _bits(gp.cpu().numpy(), pts16, "pipeline, 16 bit: points")
    _bits(gk.cpu().numpy(), keep16, "pipeline, 16 bit: keep")
    assert cloud.count() == int(keep16.sum()) == n_valid


def test_update_from_depth_in_one_graph(fresh_world, tmp_path, torch_cuda):
    """One graph holds update_from_depth and one cloud_validity call; it is replayed with the depth tensor, the pose and q0 rewritten
    in place, and each replay equals the eager result for the same inputs (and the restatement's)."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, alive, q0 = dc.robot("c1", True, tmp_path)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    q = _rows("c1", chain)
    base = sm.links[sm.rshape_link[0]]
    shapes = [s for s in range(sm.n_rshapes) if sm.links[sm.rshape_link[s]]._name != base._name]
    cams = [CAM.copy() for _ in range(3)]
    cams[1][:3, 3] = [-1.5, -0.05, 0.6]
    cams[2][:3, 3] = [-1.7, 0.1, 0.5]
    q0s = [q0, sample_q(chain, 4, seed=5)[1], sample_q(chain, 4, seed=5)[3]]
    frames = [_frame("c1", sm, q0s[k], cams[k]) for k in range(3)]
    intr = frames[0][1]
    box = ([-0.7, -0.7, 0.0], [0.7, 0.7, 1.3])

    def make():
        return PointCloud(np.zeros((0, 3)), RADIUS, bounds=box, capacity=H * W)
    eager = []
    for k in range(3):
        c = make()
        c.update_from_depth(frames[k][0], intr, cams[k], arm=arm, q=q0s[k], padding=PAD, ignore_links=[base], frame="numbotics")
        eager.append(dev.cloud_validity(c, q, PAD, shapes=shapes))
        pts, keep, n_valid = _pipeline_ref(sm, frames[k][0], intr, cams[k], q0s[k], shapes)
        assert np.array_equal(eager[k], cloud_mask(sm, pts[keep], RADIUS, q, PAD, shapes)), f"eager frame {k}"
        assert eager[k].any() and not eager[k].all(), f"frame {k}: {eager[k].mean():.3f} of the rows collide"
    assert len({e.tobytes() for e in eager}) == 3, "the three frames must differ"
    dt = torch.from_numpy(frames[0][0]).cuda()
    Tt = torch.from_numpy(cams[0]).cuda()
    qt0 = torch.from_numpy(q0s[0]).cuda()
    qt = torch.from_numpy(q).cuda()
    cloud = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # warm-up outside the capture: the staging tensors are allocated here, once
        cloud.update_from_depth(dt, intr, Tt, arm=arm, q=qt0, padding=PAD, ignore_links=[base], frame="numbotics")
        dev.cloud_validity(cloud, qt, PAD, shapes=shapes)
        side.synchronize()
        stage = cloud._stage.pts.data_ptr()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cloud.update_from_depth(dt, intr, Tt, arm=arm, q=qt0, padding=PAD, ignore_links=[base], frame="numbotics")
            mask = dev.cloud_validity(cloud, qt, PAD, shapes=shapes)
    torch.cuda.current_stream().wait_stream(side)
    assert cloud._stage.pts.data_ptr() == stage, "the captured call reused the staging tensors"
    for k in (1, 2):
        dt.copy_(torch.from_numpy(frames[k][0]).cuda())
        Tt.copy_(torch.from_numpy(cams[k]).cuda())
        qt0.copy_(torch.from_numpy(q0s[k]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(mask.cpu().numpy(), eager[k]), f"replay {k}"
    assert cloud.status() == 0


# ---- 7. the stage follows the frame and the arm -----------------------------------------------------------------------------------
def _small_frame(Hs, Ws, hole):
    """An (Hs, Ws) float32 frame of six depths with one hole, and its intrinsics."""
    d = np.linspace(0.5, 1.5, Hs * Ws).astype(np.float32)
    d[hole] = 0.0
    return np.ascontiguousarray(d.reshape(Hs, Ws)), dc.intrinsics(Hs, Ws)


def test_frame_shape_change_remakes_the_stage(torch_cuda):
    """A 3x2 host frame, then 2x3 ones -- the same pixel count, another shape -- through one cloud of capacity 6: each call leaves
    what ``backproject`` gives for that frame alone, and the third call reuses the staging tensors of the second.  The same through
    ``integrate_depth``, against the restatement of tests/cloud_fuse_cases.py."""
    from numbotics_amd.physics import PointCloud, backproject
    T = dc.camera_pose()
    box = ([-3.0, -3.0, -3.0], [3.0, 3.0, 3.0])
    frames = [_small_frame(3, 2, 1), _small_frame(2, 3, 4), _small_frame(2, 3, 2)]
    cloud = PointCloud(np.zeros((0, 3)), RADIUS, bounds=box, capacity=6)
    ptrs = []
    for k, (d, intr) in enumerate(frames):
        gp, gk = cloud.update_from_depth(d, intr, T)
        bp, bk = backproject(d, intr, T)
        rp, rk = dc.backproject_ref(d, intr, T)
        assert rk.sum() == 5, "one hole in six pixels"
        _bits(bk.cpu().numpy(), rk, f"frame {k}: backproject keep")
        _bits(gk.cpu().numpy(), bk.cpu().numpy(), f"frame {k}: keep")
        _bits(gp.cpu().numpy(), bp.cpu().numpy(), f"frame {k}: points")
        _bits(gp.cpu().numpy(), rp, f"frame {k}: points against the restatement")
        assert cloud.count() == int(rk.sum()) and cloud.status() == 0 and cloud.n == 6
        ptrs.append((gp.data_ptr(), gk.data_ptr()))
    assert ptrs[2] == ptrs[1], "the same shape again: nothing is re-made"
    fused = PointCloud(np.zeros((0, 3)), RADIUS, bounds=box, capacity=6)
    store = fc.empty_store(6)
    for k, (d, intr) in enumerate(frames):
        store, counts, _, _ = fc.integrate_ref(store, d, intr, T, RADIUS, 0.05, 0, RADIUS)
        sp, sk = fused.integrate_depth(d, intr, T, carve_margin=0.05, carve_window=0)
        _bits(sk.cpu().numpy(), store[1], f"fused frame {k}: store mask")
        _bits(sp.cpu().numpy(), store[0], f"fused frame {k}: store points")
        mc = fused.map_counts()
        assert [mc["held"], mc["appended"], mc["dropped"]] == counts.tolist() and fused.count() == mc["held"], (k, mc, counts)
        ptrs.append(fused._stage.pts.data_ptr())
    assert ptrs[-1] == ptrs[-2], "the same shape again: nothing is re-made"


def test_two_robots_filter_one_cloud(tmp_path, torch_cuda):
    """One cloud, two arms of 9 and 16 joints, q from the host: the stage's q follows the arm, and each call's mask is the one
    ``arm.cloud_self_filter`` gives directly."""
    from numbotics_amd.physics import PointCloud, backproject
    cloud = PointCloud(np.zeros((0, 3)), RADIUS, bounds=([-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]), capacity=H * W)
    robots = []
    for name in ("k9", "k16"):
        arm, chain, alive = lc.case(name, tmp_path)
        sm, _ = arm._scene_device()
        robots.append((name, arm, chain, alive, sm, lc.sample(chain, 4, 5)[2]))
    assert [r[2].dof for r in robots] == [9, 16]
    for name, arm, chain, alive, sm, q0 in robots + robots[:1]:
        depth, intr = _frame(name, sm, q0)
        bp, bk = backproject(depth, intr, CAM, frame="numbotics")
        ref = arm.cloud_self_filter(bp, q0, RADIUS, PAD, keep=bk.clone()).cpu().numpy()
        seen = bk.cpu().numpy()
        assert 0 < ref.sum() < seen.sum(), f"{name}: the filter removes {seen.sum() - ref.sum()} of {seen.sum()} pixels -- not a mixed case"
        gp, gk = cloud.update_from_depth(depth, intr, CAM, arm=arm, q=q0, padding=PAD, frame="numbotics")
        _bits(gk.cpu().numpy(), ref, f"{name}: keep")
        _bits(gp.cpu().numpy(), bp.cpu().numpy(), f"{name}: points")
        assert cloud.count() == int(ref.sum()) and not arm.in_collision_with_cloud(q0, cloud, PAD)
