"""Fused frames on the device (nbk_frame_cloud_carve, nbk_frame_cloud_novel, nbk_frame_cloud_append; carve, PointCloud.novel, append,
PointCloud.integrate_depth / map_counts / reset_map): each of the three new steps bit for bit its NumPy restatement
(tests/cloud_fuse_cases.py), the whole call bit for bit their composition over several frames of an analytic scene -- eagerly and in a
replayed graph.  Masks, indices and copies of doubles: everything is compared for equality.  Needs a real MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from numbotics_amd.scenes import sample_q
from test_gpu_parity import assert_bitwise, torch_cuda      # noqa: F401  (fixture)
import cloud_depth_cases as dc
import cloud_fuse_cases as fc


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    assert a.tobytes() == b.tobytes(), f"{what}: bits differ at {np.flatnonzero(np.asarray(a != b).reshape(a.shape[0], -1).any(axis=1))[:8]}"


# ---- 1. carve ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [k for k, _ in fc.KINDS])
def test_carve_bitwise(torch_cuda, kind):
    torch = torch_cuda
    from numbotics_amd.physics.pointcloud import carve
    opts = dict(z_min=dc.Z_MIN, z_max=dc.Z_MAX)
    for H, W in dc.SHAPES:
        d, intr, T, scale, pts, keep = fc.carve_case(H, W, kind)
        T2 = T.copy()
        T2[:3, 3] += 0.2 * T[:3, 2] + 0.03 * T[:3, 0]               # 0.2 m nearer and a little to the side: other points are in front
        dt = torch.from_numpy(d.view(np.int16) if kind == "u16" else d).cuda()
        pt = torch.from_numpy(pts).cuda()
        Tt = torch.from_numpy(np.ascontiguousarray(T)).cuda()
        for window in fc.WINDOWS:
            what = f"{W}x{H} {kind} window {window}"
            ref = fc.carve_ref(pts, keep, d, intr, T, fc.MARGIN, window, scale, dc.Z_MIN, dc.Z_MAX)
            f = fc.carved_fraction(keep, ref)
            print(f"{what}: the reference carves {f:.3f}")
            if window in fc.BANDED.get((H, W), ()):
                fc.in_band(keep, ref, what)
            if not fc.window_fits(H, W, window):
                assert f == 0.0, what
            got = carve(pts, keep, d, intr, T, fc.MARGIN, window, depth_scale=scale, **opts)
            assert got.is_cuda and got.dtype == torch.uint8
            _bits(got.cpu().numpy(), ref, what)
            # the image, the pose and the mask on the device; the mask is worked on in place, the pose rewritten between two calls
            kt = torch.from_numpy(keep.copy()).cuda()
            Tt.copy_(torch.from_numpy(np.ascontiguousarray(T)).cuda())
            assert carve(pt, kt, dt, intr, Tt, fc.MARGIN, window, depth_scale=scale, **opts) is kt
            _bits(kt.cpu().numpy(), ref, what + " (device image)")
            Tt.copy_(torch.from_numpy(np.ascontiguousarray(T2)).cuda())
            kt.copy_(torch.from_numpy(keep.copy()).cuda())
            carve(pt, kt, dt, intr, Tt, fc.MARGIN, window, depth_scale=scale, **opts)
            ref2 = fc.carve_ref(pts, keep, d, intr, T2, fc.MARGIN, window, scale, dc.Z_MIN, dc.Z_MAX)
            _bits(kt.cpu().numpy(), ref2, what + " (pose rewritten)")
            if (H, W) == (17, 33):
                assert not np.array_equal(ref, ref2), "the second pose carves other points"
        _bits(pt.cpu().numpy(), pts, "the stored points are not written")
    # an empty store and an empty image
    d, intr, T, scale, pts, keep = fc.carve_case(5, 7, kind)
    assert carve(pts[:0], keep[:0], d, intr, T, fc.MARGIN, 0, depth_scale=scale).shape == (0,)
    got = carve(pts, keep, d[:0], intr, T, fc.MARGIN, 0, depth_scale=scale)
    _bits(got.cpu().numpy(), keep, "no image: nothing is seen through")


# ---- 2. novelty ----------------------------------------------------------------------------------------------------------------------
def _novel_inputs():
    """(cloud points (561, 3), their mask, the submission (561, 3), its mask): the 33x17 surface frame, and the same image seen from
    a camera shifted by 0.06 m along its x axis."""
    d, intr, T, scale, _, _ = fc.carve_case(17, 33, "f32")
    c, ck = dc.backproject_ref(d, intr, T, scale, dc.Z_MIN, dc.Z_MAX)
    T2 = T.copy()
    T2[:3, 3] += 0.06 * T[:3, 0]
    p, pk = dc.backproject_ref(d, intr, T2, scale, dc.Z_MIN, dc.Z_MAX)
    return c, ck, p, pk


def test_novel_bitwise(torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    c, ck, p, pk = _novel_inputs()
    live = c[ck != 0]
    lo, hi = live.min(axis=0), live.max(axis=0)
    mid = 0.5 * (lo + hi)
    refs = {m: fc.novel_ref(live, p, pk, m) for m in (0.01, 0.02, 0.04)}
    share = {m: 1.0 - refs[m].sum() / pk.sum() for m in refs}
    print("novelty: dropped shares", share)
    assert 0.05 <= share[0.02] <= 0.95, f"merge 0.02: the reference drops {share[0.02]:.3f} -- not a mixed case"
    assert share[0.01] <= share[0.02] <= share[0.04]
    pt = torch.from_numpy(p).cuda()
    for m in (0.01, 0.02, 0.04):
        grids = {"one cell": dict(bounds=(lo, hi), cell=10.0),
                 "half the points in the box": dict(bounds=(lo, np.array([mid[0], hi[1], hi[2]])), cell=0.05),
                 "cell of merge / 3": dict(bounds=(mid - 0.2, mid + 0.2), cell=m / 3.0)}
        for name, kw in grids.items():
            cloud = PointCloud(c, 0.01, **kw)
            cloud.update(c, keep=ck)
            if name == "one cell":
                assert tuple(cloud.dims) == (1, 1, 1)
            if name == "half the points in the box":
                inside = float(np.mean(live[:, 0] <= mid[0]))
                assert 0.2 <= inside <= 0.8, inside
            what = f"merge {m}, {name} {tuple(int(x) for x in cloud.dims)}"
            got = cloud.novel(p, pk, m)
            _bits(got.cpu().numpy(), refs[m], what)
            kt = torch.from_numpy(pk.copy()).cuda()
            assert cloud.novel(pt, kt, m) is kt
            _bits(kt.cpu().numpy(), refs[m], what + " (in place)")
            # a held mask that hides every second slot
            held = ck.copy()
            held[::2] = 0
            ref_h = fc.novel_ref(c[held != 0], p, pk, m)
            _bits(cloud.novel(p, pk, m, held=torch.from_numpy(held).cuda()).cpu().numpy(), ref_h, what + " (held)")
            if m == 0.02:
                assert not np.array_equal(ref_h, refs[m]), "the held mask matters"
            for n in (0, 1, 63, 64, 65, 257):
                _bits(cloud.novel(p[:n], pk[:n], m).cpu().numpy(), refs[m][:n], what + f" N = {n}")
            _bits(cloud.novel(p, pk, 0.0).cpu().numpy(), pk, what + ": merge 0 drops nothing")
            _bits(cloud.novel(p, pk, -1.0).cpu().numpy(), pk, what + ": a negative merge drops nothing")
    _bits(pt.cpu().numpy(), p, "the submission is not written")
    # a submission that came in with zeros: they stay zero
    cloud = PointCloud(c, 0.01, bounds=(lo, hi))
    cloud.update(c, keep=ck)
    k0 = pk.copy()
    k0[::3] = 0
    _bits(cloud.novel(p, k0, 0.02).cpu().numpy(), fc.novel_ref(live, p, k0, 0.02), "zeros stay")
    # strict: exactly merge apart is not dropped, an identical point is; a NaN point keeps its 1
    one = PointCloud(np.array([[0.25, -0.5, 1.0]]), 0.01, bounds=([0.0, -1.0, 0.0], [1.0, 1.0, 2.0]))
    sub = np.array([[0.25 + 0.03125, -0.5, 1.0], [0.25, -0.5, 1.0], [0.25, -0.5 - 0.03125, 1.0], [0.25, -0.5, 1.0 + 0.03124], [np.nan, -0.5, 1.0],
                    [0.25, np.inf, 1.0]])
    got = one.novel(sub, np.ones(6, dtype=np.uint8), 0.03125).cpu().numpy()
    assert got.tolist() == [1, 0, 1, 0, 1, 1] and got.tolist() == fc.novel_ref(np.array([[0.25, -0.5, 1.0]]), sub, np.ones(6, np.uint8), 0.03125).tolist()
    # an empty cloud and a cloud whose status is set leave keep as it is
    empty = PointCloud(np.zeros((0, 3)), 0.01, bounds=(lo, hi), capacity=c.shape[0])
    _bits(empty.novel(p, pk, 0.04).cpu().numpy(), pk, "an empty cloud")
    empty.update(c, keep=np.zeros(c.shape[0], dtype=bool))
    _bits(empty.novel(p, pk, 0.04).cpu().numpy(), pk, "a cloud with nothing kept")
    bad = live.copy()
    bad[3, 1] = np.nan
    sick = PointCloud(live, 0.01, bounds=(lo, hi))
    sick.update(bad)
    assert sick.status() == 2
    _bits(sick.novel(p, pk, 0.04).cpu().numpy(), pk, "a cloud whose status is set")
    sick.update(live)
    _bits(sick.novel(p, pk, 0.04).cpu().numpy(), refs[0.04], "and after a clean update")
    with pytest.raises(ValueError):
        cloud.novel(p, pk, 0.02, held=torch.zeros((3,), dtype=torch.uint8, device="cuda"))


# ---- 3. append -----------------------------------------------------------------------------------------------------------------------
def _stores(M, N, rng):
    """name -> store mask (M,) uint8"""
    out = {"full": np.ones(M, np.uint8), "empty": np.zeros(M, np.uint8), "half": (rng.uniform(size=M) < 0.5).astype(np.uint8)}
    few = np.ones(M, np.uint8)
    few[rng.permutation(M)[:max(1, min(M, N // 3))]] = 0          # fewer free slots than new points (for N >= 3)
    out["few free"] = few
    end = np.ones(M, np.uint8)
    end[max(0, M - 3):] = 0
    out["free at the far end"] = end
    seams = np.ones(M, np.uint8)
    seams[[s for s in (255, 256, 1023, 1024) if s < M]] = 0
    out["free at block seams"] = seams
    return out


def test_append_bitwise(torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics.pointcloud import append, append_workspace_bytes
    rng = np.random.default_rng(5)
    seen = set()
    for M in (1, 255, 256, 257, 1025, 4099):
        store = rng.standard_normal((M, 3))
        for N in (0, 1, 64, 257):
            new = rng.standard_normal((N, 3))
            nk = (rng.uniform(size=N) < 0.7).astype(np.uint8)
            if N == 1:
                nk[:] = 1
            ws = torch.empty((append_workspace_bytes(M, N),), dtype=torch.uint8, device="cuda")
            for name, sk in _stores(M, N, rng).items():
                what = f"M = {M}, N = {N}, {name}"
                rp, rk, rc, rs = fc.append_ref(store, sk, new, nk)
                seen.add((rc[1] > 0, rc[2] > 0))
                spt, skt = torch.from_numpy(store.copy()).cuda(), torch.from_numpy(sk.copy()).cuda()
                npt, nkt = torch.from_numpy(new).cuda(), torch.from_numpy(nk).cuda()
                slot_of = torch.full((N,), 7, dtype=torch.int32, device="cuda")
                counts = torch.full((3,), -5, dtype=torch.int64, device="cuda")
                assert append(spt, skt, npt, nkt, counts=counts, slot_of=slot_of, workspace=ws) is counts
                _bits(counts.cpu().numpy(), rc, what + ": counts")
                _bits(skt.cpu().numpy(), rk, what + ": store mask")
                _bits(spt.cpu().numpy(), rp, what + ": store points")
                _bits(slot_of.cpu().numpy(), rs, what + ": slot_of")
                _bits(npt.cpu().numpy(), new, what + ": the new points are not written")
                _bits(nkt.cpu().numpy(), nk, what + ": the new mask is not written")
                assert int(rk.sum()) == rc[0] and rc[1] + rc[2] == int(nk.sum())
            # without slot_of, counts and workspace of the caller's
            sk = _stores(M, N, rng)["half"]
            rp, rk, rc, rs = fc.append_ref(store, sk, new, nk)
            spt, skt = torch.from_numpy(store.copy()).cuda(), torch.from_numpy(sk.copy()).cuda()
            counts = append(spt, skt, new, nk)
            _bits(counts.cpu().numpy(), rc, f"M = {M}, N = {N}: counts (own workspace)")
            _bits(spt.cpu().numpy(), rp, f"M = {M}, N = {N}: store points (own workspace)")
    assert seen == {(False, False), (True, False), (False, True), (True, True)}, f"appended / dropped cases seen: {seen}"


# ---- 4. the whole call ---------------------------------------------------------------------------------------------------------------
H, W = 17, 33
RADIUS, PAD, MERGE = 0.01, 0.02, 0.02
CARVE = dict(carve_margin=0.05, carve_window=1)
BOX = ([-0.7, -0.8, 0.0], [0.7, 0.8, 1.2])
CAPACITY = 4099


def _intr():
    from numbotics_amd.physics import intrinsics_from_fov
    return intrinsics_from_fov(W, H, 50.0)


def _step_ref(store, depth, T, **kw):
    return fc.integrate_ref(store, depth, _intr(), T, RADIUS, CARVE["carve_margin"], CARVE["carve_window"], MERGE, **kw)


def _make(capacity=CAPACITY):
    from numbotics_amd.physics import PointCloud
    return PointCloud(np.zeros((0, 3)), RADIUS, bounds=BOX, capacity=capacity)


def _same_clearance(dev, cloud, sp, sk, q, shapes, what):
    """cloud_clearance of the map equals that of a fresh cloud of the kept slots, with point indices mapped through the slot list."""
    from numbotics_amd.physics import PointCloud
    slots = np.flatnonzero(sk)
    fresh = PointCloud(sp[slots], RADIUS, bounds=BOX)
    d, s, p = dev.cloud_clearance(cloud, q, 0.3, shapes=shapes)
    df, sf, pf = dev.cloud_clearance(fresh, q, 0.3, shapes=shapes)
    assert_bitwise(d, df, what + ": clearance")
    assert np.array_equal(s, sf)
    near = pf >= 0
    assert near.any(), what + ": no configuration is near the map"
    assert np.array_equal(p[near], slots[pf[near]]) and np.all(p[~near] == -1), what + ": a record's point is its SLOT"


def test_integrate_depth_frames(fresh_world, tmp_path, torch_cuda):
    arm, chain, alive, q0 = dc.robot("c1", True, tmp_path)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    q = sample_q(chain, 256, seed=3)
    shapes = list(range(1, sm.n_rshapes))
    intr = _intr()
    cloud = _make()
    store = fc.empty_store(CAPACITY)
    held = 0
    for k, T in enumerate(fc.POSES):
        depth = fc.render(T, intr, H, W)
        store, counts, released, _ = _step_ref(store, depth, T)
        sp, sk = cloud.integrate_depth(depth, intr, T, merge_distance=MERGE, **CARVE)
        assert tuple(sp.shape) == (CAPACITY, 3) and tuple(sk.shape) == (CAPACITY,) and sp.is_cuda and sk.is_cuda
        _bits(sk.cpu().numpy(), store[1], f"frame {k}: store mask")
        _bits(sp.cpu().numpy(), store[0], f"frame {k}: store points")
        mc = cloud.map_counts()
        assert [mc["held"], mc["appended"], mc["dropped"]] == counts.tolist(), (mc, counts)
        assert mc["held"] == held - released.shape[0] + mc["appended"] and mc["dropped"] == 0 and mc["appended"] > 0
        assert cloud.count() == mc["held"] == int(store[1].sum()) and cloud.status() == 0 and cloud.n == CAPACITY
        if k > 0:
            assert 0 < mc["appended"] < H * W, f"frame {k}: part of the frame is known already ({mc})"
        held = mc["held"]
        _same_clearance(dev, cloud, store[0], store[1], q, shapes, f"frame {k}")
    # a fourth frame, the sphere moved: the old one is seen through
    before = store
    T = fc.POSES[0]
    depth = fc.render(T, intr, H, W, sphere_c=fc.SPHERE_MOVED)
    store, counts, released, slot_of = _step_ref(store, depth, T)
    sp, sk = cloud.integrate_depth(depth, intr, T, merge_distance=MERGE, **CARVE)
    _bits(sk.cpu().numpy(), store[1], "the sphere moved: store mask")
    _bits(sp.cpu().numpy(), store[0], "the sphere moved: store points")
    got_k, got_p = sk.cpu().numpy(), sp.cpu().numpy()
    old = (before[1] != 0) & (np.linalg.norm(before[0] - fc.SPHERE_C, axis=1) <= fc.SPHERE_R + 0.01)
    through = fc.carve_ref(before[0], before[1], depth, intr, T, CARVE["carve_margin"], CARVE["carve_window"]) == 0
    gone = old & through & (before[1] != 0)
    assert gone.sum() >= 8, f"{old.sum()} slots on the old sphere, the frame sees through {gone.sum()}"
    # (a released slot may be refilled by this very frame's points, so the statement is about points, not slots)
    left = np.flatnonzero((got_k != 0) & (np.linalg.norm(got_p - fc.SPHERE_C, axis=1) <= fc.SPHERE_R + 0.01))
    assert (before[1][left] != 0).all() and np.array_equal(got_p[left], before[0][left]) and not gone[left].any(), \
        "what is still held on the old sphere was there before and is not in front of what the frame sees"
    assert left.shape[0] == old.sum() - gone.sum()
    on_new = (got_k != 0) & (np.abs(np.linalg.norm(got_p - fc.SPHERE_MOVED, axis=1) - fc.SPHERE_R) < 1e-6)
    assert on_new.sum() >= 8, f"the new sphere's points are held ({on_new.sum()})"
    mc = cloud.map_counts()
    assert released.shape[0] >= gone.sum() and mc["held"] == held - released.shape[0] + mc["appended"] == counts[0]
    _same_clearance(dev, cloud, store[0], store[1], q, shapes, "the sphere moved")
    # a plain update ends the map: the next integration starts from an empty store; so does reset_map
    cloud.update(np.zeros((3, 3)))
    assert cloud.count() == 3
    first, _, _, _ = _step_ref(fc.empty_store(CAPACITY), depth, T)
    sp, sk = cloud.integrate_depth(depth, intr, T, merge_distance=MERGE, **CARVE)
    _bits(sk.cpu().numpy(), first[1], "after a plain update: store mask")
    assert cloud.count() == int(first[1].sum()) == H * W
    cloud.integrate_depth(depth, intr, T, merge_distance=MERGE, **CARVE)
    assert cloud.map_counts() == {"held": H * W, "appended": 0, "dropped": 0}, "the same frame again brings nothing new"
    cloud.reset_map()
    cloud.integrate_depth(depth, intr, T, merge_distance=MERGE, **CARVE)
    assert cloud.map_counts() == {"held": H * W, "appended": H * W, "dropped": 0}
    # merge_distance defaults to the radius; radius 0 needs it
    from numbotics_amd.physics import PointCloud
    bare = PointCloud(np.zeros((0, 3)), 0.0, bounds=BOX, capacity=600)
    with pytest.raises(ValueError):
        bare.integrate_depth(depth, intr, T)
    with pytest.raises(TypeError):
        cloud.integrate_depth(depth, intr, T, no_such_option=1)


def test_map_lifecycle(torch_cuda):
    """integrate, integrate, update(points), integrate, reset_map(), integrate on 4x4 frames and 32 slots: after each integration the
    map is what the restatement gives for a store that started empty where the docstring says it does -- at the first call, after a
    plain update and after reset_map -- and went on from the previous frame otherwise."""
    from numbotics_amd.physics import PointCloud, intrinsics_from_fov
    h = w = 4
    intr = intrinsics_from_fov(w, h, 50.0)
    poses = (fc.POSES[0], fc.POSES[1], fc.POSES[2], fc.POSES[1])
    frames = [fc.render(T, intr, h, w) for T in poses]
    step = lambda store, k: fc.integrate_ref(store, frames[k], intr, poses[k], RADIUS, 0.05, 1, MERGE)[:2]          # noqa: E731
    cloud = PointCloud(np.zeros((0, 3)), RADIUS, bounds=BOX, capacity=32)

    def integrate(k, store, what):
        store, counts = step(store, k)
        sp, sk = cloud.integrate_depth(frames[k], intr, poses[k], merge_distance=MERGE, **CARVE)
        mc = cloud.map_counts()
        assert [mc["held"], mc["appended"], mc["dropped"]] == counts.tolist(), (what, mc, counts)
        _bits(sk.cpu().numpy(), store[1], what + ": store mask")
        # (a map that starts anew zeroes the mask, not the points: only the held slots' points are the map's)
        _bits(sp.cpu().numpy()[store[1] != 0], store[0][store[1] != 0], what + ": the held slots' points")
        assert cloud.count() == mc["held"] and cloud.n == 32
        return store, mc["held"]

    store, first = integrate(0, fc.empty_store(32), "the first call starts empty")
    store, second = integrate(1, store, "the second goes on")
    assert second > step(fc.empty_store(32), 1)[1][0] > 0 and second > first, "going on and starting anew differ"
    cloud.update(np.zeros((3, 3)))
    assert cloud.count() == 3
    went_on = step(store, 2)[1][0]
    store, third = integrate(2, fc.empty_store(32), "after a plain update: starts empty")
    assert 0 < third < went_on, "going on and starting anew differ"
    went_on = step(store, 3)[1][0]
    cloud.reset_map()
    store, fourth = integrate(3, fc.empty_store(32), "after reset_map: starts empty")
    assert 0 < fourth < went_on, "going on and starting anew differ"


def test_integrate_depth_small_store_drops(torch_cuda):
    """A capacity below the first frame's valid pixels: the surplus is dropped and counted, and the reference agrees on which."""
    intr = _intr()
    cap = 300
    cloud = _make(cap)
    store = fc.empty_store(cap)
    for k, T in enumerate(fc.POSES[:2]):
        depth = fc.render(T, intr, H, W)
        store, counts, released, slot_of = _step_ref(store, depth, T)
        sp, sk = cloud.integrate_depth(depth, intr, T, merge_distance=MERGE, **CARVE)
        _bits(sk.cpu().numpy(), store[1], f"frame {k}: store mask")
        _bits(sp.cpu().numpy(), store[0], f"frame {k}: store points")
        mc = cloud.map_counts()
        assert [mc["held"], mc["appended"], mc["dropped"]] == counts.tolist() and mc["dropped"] > 0 and mc["held"] == cap
        if k == 0:
            assert mc == {"held": cap, "appended": cap, "dropped": H * W - cap} and slot_of[:cap].tolist() == list(range(cap))
    assert cloud.count() == cap and cloud.status() == 0


ARM_SPHERE_C, ARM_SPHERE_R = np.array([-0.17, -0.12, 0.27]), 0.1


def test_integrate_depth_with_the_arm(fresh_world, tmp_path, torch_cuda):
    """With arm, q and padding: the arm's own image stays out of the frame, stored points the arm touches now are released, and the
    map reads free at q afterwards.  The scene's sphere sits on the arm, and q changes from frame to frame."""
    arm, chain, alive, q0 = dc.robot("c1", True, tmp_path)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    q = sample_q(chain, 256, seed=3)
    qs = [sample_q(chain, 4, seed=5)[1], q0, sample_q(chain, 4, seed=5)[3]]      # (the arm moves INTO the stored sphere at frame 1)
    intr = _intr()
    cloud = _make()
    store = fc.empty_store(CAPACITY)
    filtered = cleared = 0                                  # slots the two self-filter steps change; the second one's share
    for k, T in enumerate(fc.POSES):
        depth = fc.render(T, intr, H, W, sphere_c=ARM_SPHERE_C, sphere_r=ARM_SPHERE_R)
        plain, _, _, _ = _step_ref(store, depth, T)
        kept, _, _, _ = _step_ref(store, depth, T, sm=sm, q=qs[k], pad=PAD, clear_robot=False)
        store, counts, released, _ = _step_ref(store, depth, T, sm=sm, q=qs[k], pad=PAD)
        filtered += int((plain[1] != store[1]).sum())
        cleared += int((kept[1] != store[1]).sum())
        sp, sk = cloud.integrate_depth(depth, intr, T, arm=arm, q=qs[k], padding=PAD, merge_distance=MERGE, **CARVE)
        _bits(sk.cpu().numpy(), store[1], f"frame {k}: store mask")
        _bits(sp.cpu().numpy(), store[0], f"frame {k}: store points")
        mc = cloud.map_counts()
        assert [mc["held"], mc["appended"], mc["dropped"]] == counts.tolist()
        assert not arm.in_collision_with_cloud(qs[k], cloud, PAD), f"frame {k}: the map collides with the arm at the frame's q"
        _same_clearance(dev, cloud, store[0], store[1], q, None, f"frame {k} with the arm")
    print(f"with the arm: the two self-filter steps change {filtered} slots, the store's own {cleared}")
    assert filtered > 0 and cleared > 0, "the reference's self-filter steps change nothing: not a test of them"
    # clear_robot=False leaves the store's points alone
    other = _make()
    store = fc.empty_store(CAPACITY)
    for k, T in enumerate(fc.POSES[:2]):
        depth = fc.render(T, intr, H, W, sphere_c=ARM_SPHERE_C, sphere_r=ARM_SPHERE_R)
        store, counts, _, _ = _step_ref(store, depth, T, sm=sm, q=qs[k], pad=PAD, clear_robot=False)
        sp, sk = other.integrate_depth(depth, intr, T, arm=arm, q=qs[k], padding=PAD, merge_distance=MERGE, clear_robot=False, **CARVE)
        _bits(sk.cpu().numpy(), store[1], f"frame {k}, clear_robot=False: store mask")
        _bits(sp.cpu().numpy(), store[0], f"frame {k}, clear_robot=False: store points")
    with pytest.raises(ValueError):
        other.integrate_depth(depth, intr, T, arm=arm, merge_distance=MERGE)


# ---- 5. graph ------------------------------------------------------------------------------------------------------------------------
def test_integrate_depth_in_one_graph(fresh_world, tmp_path, torch_cuda):
    """One graph holds one integrate_depth (one update); it is replayed over the frames with the depth tensor, the pose and q rewritten
    in place, and the store after each replay equals the eager run's on a second cloud (and the reference's)."""
    torch = torch_cuda
    arm, chain, alive, q0 = dc.robot("c1", True, tmp_path)
    sm = arm.scene_model()
    qs = [sample_q(chain, 4, seed=5)[1], q0, sample_q(chain, 4, seed=5)[3]]      # (the arm moves INTO the stored sphere at frame 1)
    intr = _intr()
    frames = [fc.render(T, intr, H, W, sphere_c=ARM_SPHERE_C, sphere_r=ARM_SPHERE_R) for T in fc.POSES]
    kw = dict(arm=arm, padding=PAD, merge_distance=MERGE, **CARVE)
    eager_cloud = _make()
    eager = []
    store = fc.empty_store(CAPACITY)
    for k in range(3):
        sp, sk = eager_cloud.integrate_depth(frames[k], intr, fc.POSES[k], q=qs[k], **kw)
        eager.append((sp.cpu().numpy().copy(), sk.cpu().numpy().copy(), eager_cloud.map_counts()))
        store, _, _, _ = _step_ref(store, frames[k], fc.POSES[k], sm=sm, q=qs[k], pad=PAD)
        _bits(eager[k][1], store[1], f"eager frame {k}: store mask")
    assert len({e[1].tobytes() for e in eager}) == 3, "the three frames must differ"
    dt = torch.from_numpy(frames[0]).cuda()
    Tt = torch.from_numpy(np.ascontiguousarray(fc.POSES[0])).cuda()
    qt = torch.from_numpy(qs[0]).cuda()
    cloud = _make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # warm-up outside the capture: store, staging and workspace are allocated here, once, and the map starts (frame 0)
        sp, sk = cloud.integrate_depth(dt, intr, Tt, q=qt, **kw)
        side.synchronize()
        _bits(sk.cpu().numpy(), eager[0][1], "warm-up: store mask")
        ptrs = (sp.data_ptr(), sk.data_ptr(), cloud._map.ws.data_ptr(), cloud._stage.pts.data_ptr())
        dt.copy_(torch.from_numpy(frames[1]).cuda())
        Tt.copy_(torch.from_numpy(np.ascontiguousarray(fc.POSES[1])).cuda())
        qt.copy_(torch.from_numpy(qs[1]).cuda())
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            gp, gk = cloud.integrate_depth(dt, intr, Tt, q=qt, **kw)
    torch.cuda.current_stream().wait_stream(side)
    assert (gp.data_ptr(), gk.data_ptr(), cloud._map.ws.data_ptr(), cloud._stage.pts.data_ptr()) == ptrs, "the captured call allocated nothing"
    torch.cuda.synchronize()
    _bits(gk.cpu().numpy(), eager[0][1], "the capture itself runs nothing")
    for k in (1, 2):
        dt.copy_(torch.from_numpy(frames[k]).cuda())
        Tt.copy_(torch.from_numpy(np.ascontiguousarray(fc.POSES[k])).cuda())
        qt.copy_(torch.from_numpy(qs[k]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        _bits(gk.cpu().numpy(), eager[k][1], f"replay {k}: store mask")
        _bits(gp.cpu().numpy(), eager[k][0], f"replay {k}: store points")
        assert cloud.map_counts() == eager[k][2], f"replay {k}: counts"
        assert cloud.count() == eager[k][2]["held"] and cloud.status() == 0
