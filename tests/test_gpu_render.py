"""Rendered depth frames on the device (nbk_render_depth_batch; DeviceModel.render_depth, Arm.depth_images, World.depth_image): against
the analytic ray casters of tests/render_cases.py on single primitives, against the CPU oracle's distances on the arm among its
obstacles, bitwise independence of every pixel from the frame around it, the sizes, selections and edges of the contract, and the
loops the frames close: the arm's own image filtered out of what it rendered, and a captured render -> update -> validity graph.
Needs a real MI355X.

The depth bound of a hit pixel with incidence cosine cos >= 0.2 is  -t32 <= z_true - z <= eps / (L cos) + t32,  t32 = z_true 2^-23 +
1e-9: the march stops within eps of the convex body, which lies behind its tangent plane at the true hit, and a unit of depth is L
long; t32 is the float32 rounding of the output plus the accuracy of the iterative distances."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from numbotics_amd.scenes import build_scene, sample_q
from test_gpu_parity import torch_cuda      # noqa: F401  (fixture)
import render_cases as rc
import long_chain_cases as lc

EPS = rc.EPS


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{what}: bits differ"


def _render(torch, dev, q, T, intr, H, W, **kw):
    """-> depth (B, H, W) float32, label (B, H, W) int32, counts (3,) int64 as NumPy."""
    cnt = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    d, l = dev.render_depth(q, T, intr, H, W, labels=True, counts=cnt, **kw)
    assert d.is_cuda and d.dtype == torch.float32 and l.dtype == torch.int32 and tuple(d.shape) == tuple(l.shape) and d.shape[1:] == (H, W)
    d, l, cnt = d.cpu().numpy(), l.cpu().numpy(), cnt.cpu().numpy()
    assert cnt[0] == (l >= 0).sum() and cnt[1] == (l == -2).sum() and cnt[2] >= 0, "counts are the sums over the label image"
    return d, l, cnt


def _check_depth_bound(t, d, l, what, want_label):
    d, l = d.reshape(-1).astype(np.float64), l.reshape(-1)
    assert not (l == -2).any(), f"{what}: unresolved pixels"
    hit = l >= 0
    assert not ((hit != t["hit"]) & ~t["graze"]).any(), f"{what}: classes differ at {np.flatnonzero((hit != t['hit']) & ~t['graze'])[:8]}"
    assert np.all(l[hit] == want_label) and np.all(d[~hit] == 0.0), f"{what}: labels"
    ok = hit & t["hit"] & (t["cos"] >= 0.2)
    assert ok.sum() >= 27
    err = (t["z"] - d)[ok]
    t32 = t["z"][ok] * 2.0 ** -23 + 1e-9
    hi = EPS / (t["L"] * t["cos"])[ok] + t32
    print(f"{what}: {ok.sum()} pixels, z_true - z in [{err.min():.3e}, {err.max():.3e}], worst share of the bound {np.max(err / hi):.3f}")
    assert np.all(err >= -t32) and np.all(err <= hi), f"{what}: {err.min()} .. {err.max()}"


# ---- 1. analytic truth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.analytic_cases(), ids=[c[0] for c in rc.analytic_cases()])
def test_single_primitives_against_their_ray_casters(torch_cuda, case):
    from numbotics_amd.engine import DeviceModel
    name, kind, T, prm, far, cams = case
    dev = DeviceModel(rc.static_model([(kind, T, prm)]))
    intr = rc.intrinsics(rc.H1, rc.W1)
    for k, Tc in enumerate(cams):
        t = rc.truth(kind, T, prm, rc.H1, rc.W1, intr, Tc, far=far)
        rc.reference_conditions(t, f"{name} pose {k}")
        d, l, _ = _render(torch_cuda, dev, np.zeros((1, 1)), Tc, intr, rc.H1, rc.W1, far=far)
        _check_depth_bound(t, d, l, f"{name} pose {k}", 0)
        # the same camera given in the reference's frame
        d2, l2, _ = _render(torch_cuda, dev, np.zeros((1, 1)), rc.numbotics_pose(Tc), intr, rc.H1, rc.W1, far=far, frame="numbotics")
        _bits(d2, d, f"{name} pose {k}: numbotics frame")
        _bits(l2, l, f"{name} pose {k}: numbotics frame labels")


# ---- 2. oracle truth -------------------------------------------------------------------------------------------------------------------
def _check_against_oracle(sm, q, Tc, intr, d, l, drawn, near, what, in_front=True):
    """Every hit point lies on its labelled shape and in no other drawn shape; nothing drawn stands in front of any pixel."""
    from numbotics_amd.physics.pointcloud import backproject_host
    H, W = d.shape
    drawn = np.asarray(drawn)
    _, wdir, L = rc.rays(H, W, intr, Tc)
    lab = l.reshape(-1)
    hit = lab >= 0
    assert np.isin(lab[hit], drawn).all(), f"{what}: a label names a shape that is not drawn"
    pts, keep = backproject_host(d, intr, Tc)
    assert np.array_equal(keep.astype(bool), hit), f"{what}: a hit has a positive depth, a miss is a hole"
    z = d.reshape(-1).astype(np.float64)
    if hit.any():
        D = rc.oracle_distances(sm, q, pts[hit])
        t = z[hit] * 2.0 ** -23 * L[hit] + 1e-8
        own = D[np.arange(hit.sum()), lab[hit]]
        print(f"{what}: {hit.sum()} hits, own distance in [{own.min():.3e}, {own.max():.3e}], others >= {D[:, drawn].min():.3e}")
        assert np.all(own >= -t) and np.all(own <= EPS + t), f"{what}: the labelled shape is at {own.min()} .. {own.max()}"
        assert np.all(D[:, drawn] >= -t[:, None]), f"{what}: a hit point lies {D[:, drawn].min()} inside another shape"
    if in_front:
        zend = np.linalg.norm(Tc[:3, 3]) + 2.5                 # beyond every shape of these scenes
        zhi = np.where(hit, z - 4.0 * EPS / L, zend)
        sel = np.flatnonzero(lab != -2)
        u, v = rc.pixel_grid(H, W)
        zs = near + (np.arange(16)[None, :] + 0.5) / 16.0 * (zhi[sel, None] - near)
        P = rc.points_at(intr, Tc, u[sel, None], v[sel, None], zs).reshape(-1, 3)
        Df = rc.oracle_distances(sm, q, P)[:, drawn]
        print(f"{what}: {P.shape[0]} points in front, nearest shape at {Df.min():.3e}")
        assert np.all(Df > 0.0), f"{what}: a drawn shape stands {Df.min()} in front of pixel {sel[np.argmin(Df.min(1)) // 16]}"


@pytest.mark.parametrize("name", ["c2", "c2m"])
def test_arm_and_world_against_the_oracle(fresh_world, torch_cuda, name):
    arm, chain, obs = build_scene(name)
    sm, dev = arm._scene_device()
    qs = sample_q(chain, 3, seed=5)
    intr = rc.intrinsics(rc.H2, rc.W2)
    drawn = np.arange(sm.n_rshapes + sm.n_wshapes)
    kinds = set()
    for k in range(3):
        Tc = rc.arm_camera(k)
        d, l, cnt = _render(torch_cuda, dev, qs[k], Tc, intr, rc.H2, rc.W2)
        assert cnt[1] <= 0.02 * rc.H2 * rc.W2, f"{name} frame {k}: {cnt[1]} unresolved pixels"
        assert np.all(d[l < 0] == 0.0)
        assert (l >= 0).sum() >= 40 and (l == -1).sum() >= 40, f"{name} frame {k}: {np.unique(l, return_counts=True)}"
        kinds.update(int(x) for x in np.unique(l[l >= 0]))
        _check_against_oracle(sm, qs[k], Tc, intr, d[0], l[0], drawn, rc.NEAR, f"{name} frame {k}")
    assert len([s for s in kinds if s < sm.n_rshapes]) >= 4 and any(s >= sm.n_rshapes for s in kinds), f"labels seen: {sorted(kinds)}"


# ---- 3. pixel independence -----------------------------------------------------------------------------------------------------------
def test_pixels_do_not_depend_on_their_frame(fresh_world, torch_cuda):
    torch = torch_cuda
    arm, chain, obs = build_scene("c2")
    sm, dev = arm._scene_device()
    qs = sample_q(chain, 3, seed=5)
    cams = [rc.arm_camera(k) for k in range(3)]
    H, W = 17, 23
    fx = fy = 20.0
    cx, cy = 11.0, 8.0
    full = [_render(torch, dev, qs[k], cams[k], (fx, fy, cx, cy), H, W) for k in range(3)]
    assert all((f[1] >= 0).sum() >= 30 and (f[1] == -1).sum() >= 30 for f in full)
    for x0, y0, w, h in ((5, 3, 9, 8), (0, 0, 1, 1), (7, 0, 16, 17)):
        for k in range(3):
            d, l, _ = _render(torch, dev, qs[k], cams[k], (fx, fy, cx - x0, cy - y0), h, w)
            _bits(d[0], full[k][0][0, y0:y0 + h, x0:x0 + w], f"window {(x0, y0, w, h)} frame {k}: depth")
            _bits(l[0], full[k][1][0, y0:y0 + h, x0:x0 + w], f"window {(x0, y0, w, h)} frame {k}: labels")
    # batches: three frames in one call, one pose with many q, one q with many poses
    d, l, cnt = _render(torch, dev, qs, np.stack(cams), (fx, fy, cx, cy), H, W)
    assert d.shape == (3, H, W)
    for k in range(3):
        _bits(d[k], full[k][0][0], f"batch frame {k}: depth")
        _bits(l[k], full[k][1][0], f"batch frame {k}: labels")
    assert np.array_equal(cnt, sum(f[2] for f in full))
    d1, l1, _ = _render(torch, dev, qs, cams[0], (fx, fy, cx, cy), H, W)
    d2, l2, _ = _render(torch, dev, qs, np.stack([cams[0]] * 3), (fx, fy, cx, cy), H, W)
    _bits(d1, d2, "one pose, many q"); _bits(l1, l2, "one pose, many q: labels")
    _bits(d1[0], full[0][0][0], "one pose, many q: frame 0")
    assert not np.array_equal(d1[1], d1[0])
    d1, l1, _ = _render(torch, dev, qs[0], np.stack(cams), (fx, fy, cx, cy), H, W)
    d2, l2, _ = _render(torch, dev, np.stack([qs[0]] * 3), np.stack(cams), (fx, fy, cx, cy), H, W)
    _bits(d1, d2, "one q, many poses"); _bits(l1, l2, "one q, many poses: labels")
    # device tensors in, and the same call again
    qt, Tt = torch.from_numpy(qs).cuda(), torch.from_numpy(np.ascontiguousarray(np.stack(cams)[:, :3, :])).cuda()
    for _ in range(2):
        dd, ll, cc = _render(torch, dev, qt, Tt, (fx, fy, cx, cy), H, W)
        _bits(dd, d, "device inputs / repeated call: depth"); _bits(ll, l, "labels"); assert np.array_equal(cc, cnt)


# ---- 4. sizes and selections ---------------------------------------------------------------------------------------------------------
def test_frame_sizes(fresh_world, torch_cuda):
    arm, chain, obs = build_scene("c2")
    sm, dev = arm._scene_device()
    q = sample_q(chain, 3, seed=5)[0]
    Tc = rc.arm_camera(0)
    intr = (40.0, 40.0, 20.0, 30.0)
    ref = _render(torch_cuda, dev, q, Tc, intr, 70, 70)
    assert (ref[1] >= 0).sum() > 200 and (ref[1] == -1).sum() > 200
    for H, W in ((1, 1), (1, 64), (3, 70), (8, 8), (9, 13), (65, 2)):
        d, l, _ = _render(torch_cuda, dev, q, Tc, intr, H, W)
        _bits(d[0], ref[0][0, :H, :W], f"{W}x{H}: depth")
        _bits(l[0], ref[1][0, :H, :W], f"{W}x{H}: labels")
    for H, W in ((0, 5), (5, 0)):
        d, l, cnt = _render(torch_cuda, dev, q, Tc, intr, H, W)
        assert d.size == 0 and np.array_equal(cnt, [0, 0, 0])
    # nothing selected and no world: every pixel is a miss, with the caller's value
    d, l, cnt = _render(torch_cuda, dev, q, Tc, intr, 9, 13, shapes=[], world=False, miss=-1.5)
    assert np.all(d == np.float32(-1.5)) and np.all(l == -1) and np.array_equal(cnt, [0, 0, 0])


def test_selections_hide_exactly_their_shapes(fresh_world, torch_cuda):
    arm, chain, obs = build_scene("c2")
    sm, dev = arm._scene_device()
    q = sample_q(chain, 3, seed=5)[0]
    P = rc.numbotics_pose(rc.arm_camera(0))
    H, W = rc.H2, rc.W2
    d_all, l_all = arm.depth_images(q, P, W, H, labels=True)
    assert d_all.shape == (H, W) and isinstance(d_all, np.ndarray) and d_all.dtype == np.float32
    seen = [s for s in np.unique(l_all) if 0 <= s < sm.n_rshapes]
    assert len(seen) >= 3 and (l_all >= sm.n_rshapes).any()
    link = sm.links[sm.rshape_link[seen[len(seen) // 2]]]
    of_link = [s for s in range(sm.n_rshapes) if sm.rshape_link[s] == sm.rshape_link[seen[len(seen) // 2]]]
    d_ig, l_ig = arm.depth_images(q, P, W, H, labels=True, ignore_links=[link])
    assert not np.isin(l_ig, of_link).any() and np.isin(l_all, of_link).any()
    same = ~np.isin(l_all, of_link)
    assert np.array_equal(l_ig[same], l_all[same]), "a pixel that did not show the hidden link keeps its label"
    d_on, l_on = arm.depth_images(q, P, W, H, labels=True, links=[link._name], world=False)
    assert set(np.unique(l_on)) <= set(of_link) | {-1, -2} and np.isin(l_on, of_link).any()
    assert np.array_equal(np.isin(l_on, of_link) | ~np.isin(l_all, of_link), np.ones_like(l_on, dtype=bool)), "the link alone covers what it showed"
    d_nw, l_nw = arm.depth_images(q, P, W, H, labels=True, world=False)
    assert not (l_nw >= sm.n_rshapes).any()
    _check_against_oracle(sm, q, rc.arm_camera(0), rc.intrinsics(H, W), d_ig, l_ig,
                          [s for s in range(sm.n_rshapes + sm.n_wshapes) if s not in of_link], rc.NEAR, "ignore_links")


def test_more_than_64_robot_shapes(torch_cuda):
    import cloud_ladder_cases as clc
    from numbotics_amd.engine import DeviceModel
    rb = clc.robot("s72")
    sm = rb.sm
    assert sm.n_rshapes == 72
    dev = DeviceModel(sm)
    q = rb.q[3]
    Tc = rc.robot_view(sm, q, 1.0)
    intr = rc.intrinsics(rc.H2, rc.W2)
    drawn = np.arange(sm.n_rshapes + sm.n_wshapes)
    d, l, cnt = _render(torch_cuda, dev, q, Tc, intr, rc.H2, rc.W2)
    assert (l >= 0).sum() >= 30 and (l == -1).sum() >= 30 and cnt[1] <= 0.02 * l.size, np.unique(l, return_counts=True)
    _check_against_oracle(sm, q, Tc, intr, d[0], l[0], drawn, rc.NEAR, "s72")
    # a selection across the words of the shape mask, in the caller's numbering
    sel = [s for s in range(72) if s % 3 != 1]
    d, l, _ = _render(torch_cuda, dev, q, Tc, intr, rc.H2, rc.W2, shapes=sel, world=False)
    assert set(np.unique(l)) <= set(sel) | {-1, -2} and (l >= 0).sum() >= 20
    _check_against_oracle(sm, q, Tc, intr, d[0], l[0], sel, rc.NEAR, "s72 selection")


def test_world_of_70_small_spheres(torch_cuda):
    """Seventy spheres on a grid in front of the camera: the tile cull takes the drawn shapes 64 at a time."""
    from numbotics_amd.engine import DeviceModel
    rng = np.random.default_rng(70)
    gx, gy = np.meshgrid(np.arange(10), np.arange(7))
    c = np.stack((0.22 * (gx.ravel() - 4.5), 0.22 * (gy.ravel() - 3.0), 2.0 + rng.uniform(-0.3, 0.3, 70)), 1)
    r = rng.uniform(0.04, 0.09, 70)
    recs = [(rc.SH_SPHERE, rc._pose((0, 0, 0), c[i]), np.array([r[i], 0, 0, 0.0])) for i in range(70)]
    dev = DeviceModel(rc.static_model(recs))
    H, W = 36, 48
    intr = rc.intrinsics(H, W)
    Tc = np.eye(4)
    ts = [rc.truth(rc.SH_SPHERE, recs[i][1], recs[i][2], H, W, intr, Tc) for i in range(70)]
    Z = np.stack([t["z"] for t in ts])
    first = Z.argmin(0)
    t = {k: np.stack([tt[k] for tt in ts])[first, np.arange(H * W)] for k in ("z", "hit", "cos", "L")}
    t["graze"] = np.stack([tt["graze"] for tt in ts]).any(0)
    assert len(np.unique(first[t["hit"]])) >= 60 and t["hit"].sum() >= 200 and (~t["hit"]).sum() >= 200
    d, l, _ = _render(torch_cuda, dev, np.zeros((1, 1)), Tc, intr, H, W)
    lab = l.reshape(-1)
    both = (lab >= 0) & t["hit"] & ~t["graze"]
    assert np.array_equal(lab[both], first[both]) and (lab[both] >= 64).any()
    _check_depth_bound(t, d, np.where(l >= 0, 0, l), "70 spheres", 0)


# ---- 5. edges of the contract ----------------------------------------------------------------------------------------------------------
def test_contract_edges(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.engine import DeviceModel
    intr = rc.intrinsics(9, 13)
    q0 = np.zeros((1, 1))
    I = np.eye(4)
    # the camera inside a box: every pixel is the near plane
    dev = DeviceModel(rc.static_model([(rc.SH_BOX, rc._pose((0.3, 0.2, 0.1), [0.05, 0.0, 0.1]), np.array([0.5, 0.6, 0.7, 0.0]))]))
    d, l, cnt = _render(torch, dev, q0, I, intr, 9, 13, near=0.02)
    assert np.all(d == np.float32(0.02)) and np.all(l == 0) and cnt[0] == 117
    # a sphere the near plane cuts: inside the cut the depth is the near plane's, around it the sphere's own
    sph = (rc.SH_SPHERE, rc._pose((0, 0, 0), rc.CENTRE), np.array([0.15, 0, 0, 0.0]))
    dev = DeviceModel(rc.static_model([sph]))
    H, W = rc.H1, rc.W1
    intr = rc.intrinsics(H, W)
    near = 1.2
    d, l, _ = _render(torch, dev, q0, I, intr, H, W, near=near)
    o, w, L = rc.rays(H, W, intr, I)
    sd_near = rc.sd_shape(*sph, o + near * w)
    t = rc.truth(*sph, H, W, intr, I, near=0.0)
    cut = sd_near < -2 * EPS
    assert cut.sum() >= 10 and np.all(d.reshape(-1)[cut] == np.float32(near)) and np.all(l.reshape(-1)[cut] == 0)
    rim = t["hit"] & (sd_near > 2 * EPS) & (t["z"] > near) & (t["cos"] >= 0.2)
    assert rim.sum() >= 5
    err = (t["z"] - d.reshape(-1))[rim]
    assert np.all(err >= -(t["z"][rim] * 2.0 ** -23 + 1e-9)) and np.all(err <= EPS / (t["L"] * t["cos"])[rim] + t["z"][rim] * 2.0 ** -23 + 1e-9)
    # a surface beyond far: a miss
    d, l, cnt = _render(torch, dev, q0, I, intr, H, W, far=1.1)
    assert np.all(l == -1) and np.all(d == 0.0)
    # planes: a ray parallel to one, and one behind the camera.  The camera looks along the world's x axis (exact zeros in its
    # pose); with an odd height the middle row is horizontal
    cam = np.eye(4)
    ground = (rc.SH_PLANE, rc._pose((0, 0, 0), [0.0, 0.0, -1.0]), np.array([0.0, 0.0, 1.0, 0.0]))
    back = (rc.SH_PLANE, rc._pose((0, 0, 0), [-1.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0, 0.0]))
    dev = DeviceModel(rc.static_model([back, ground]))
    intr = rc.intrinsics(9, 13)
    d, l, _ = _render(torch, dev, q0, cam, intr, 9, 13, frame="numbotics")
    assert np.all(l[0, :5] == -1) and np.all(l[0, 5:] == 1), l[0]
    v = np.arange(5, 9, dtype=np.float64)
    assert np.allclose(d[0, 5:, 6], 1.0 / ((v - intr[3]) / intr[1]), rtol=2e-7)
    # max_steps = 1: what one distance evaluation does not decide is unresolved, and counted
    arm, chain, obs = build_scene("c2")
    sm, dev = arm._scene_device()
    qs = sample_q(chain, 3, seed=5)
    Tc = rc.arm_camera(0)
    intr = rc.intrinsics(rc.H2, rc.W2)
    d, l, cnt = _render(torch, dev, qs[0], Tc, intr, rc.H2, rc.W2, max_steps=1)
    assert cnt[1] >= 30 and np.all(d[l == -2] == 0.0)
    # a non-finite q row: that frame is unresolved in every pixel, the others are as alone
    bad = qs.copy()
    bad[1, 2] = np.nan
    d, l, cnt = _render(torch, dev, bad, Tc, intr, rc.H2, rc.W2, miss=-1.0)
    assert np.all(l[1] == -2) and np.all(d[1] == -1.0)
    for k in (0, 2):
        dk, lk, _ = _render(torch, dev, qs[k], Tc, intr, rc.H2, rc.W2, miss=-1.0)
        _bits(d[k], dk[0], f"frame {k} beside a non-finite one"); _bits(l[k], lk[0], "labels")
    Tb = np.stack([Tc] * 3)
    Tb[2, 1, 3] = np.inf
    d, l, cnt = _render(torch, dev, qs, Tb, intr, rc.H2, rc.W2)
    assert np.all(l[2] == -2) and not (l[0] == -2).all()


def test_movable_world_and_its_status(fresh_world, torch_cuda):
    """A movable descriptor renders what an ordinary one does, follows its obstacles, and while its world status is set every pixel
    is unresolved (the rule of the collision entries' guard)."""
    from numbotics_amd.engine import DeviceModel
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    q = sample_q(chain, 3, seed=5)[0]
    Tc = rc.arm_camera(0)
    intr = rc.intrinsics(rc.H2, rc.W2)
    fixed, mov = DeviceModel(sm), DeviceModel(sm, movable=True, world_radius=10.0)
    d0, l0, c0 = _render(torch_cuda, fixed, q, Tc, intr, rc.H2, rc.W2)
    d1, l1, c1 = _render(torch_cuda, mov, q, Tc, intr, rc.H2, rc.W2)
    _bits(d1, d0, "movable: depth"); _bits(l1, l0, "movable: labels"); assert np.array_equal(c0, c1)
    assert (l0 >= sm.n_rshapes).sum() >= 20
    poses = np.array(sm.wshape_pose, dtype=np.float64).reshape(-1, 12)
    away = poses.copy()
    away[:, 7] += 5.0                                # the obstacle leaves the view
    mov.set_world_poses(away)
    d2, l2, _ = _render(torch_cuda, mov, q, Tc, intr, rc.H2, rc.W2)
    assert not (l2 >= sm.n_rshapes).any() and np.array_equal(l2[l0 < sm.n_rshapes], l0[l0 < sm.n_rshapes])
    bad = poses.copy()
    bad[0, 3] = np.nan
    mov.set_world_poses(bad)
    assert mov.world_status() == 2
    d3, l3, c3 = _render(torch_cuda, mov, q, Tc, intr, rc.H2, rc.W2, miss=-2.0)
    assert np.all(l3 == -2) and np.all(d3 == -2.0) and np.array_equal(c3, [0, l3.size, 0])
    mov.set_world_poses(poses)
    d4, l4, c4 = _render(torch_cuda, mov, q, Tc, intr, rc.H2, rc.W2)
    _bits(d4, d0, "status cleared: depth"); _bits(l4, l0, "status cleared: labels")


# ---- 6. closed loops -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2", "k16"])
def test_the_arm_filters_out_what_it_rendered(fresh_world, tmp_path, torch_cuda, name):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    if name == "c2":
        arm, chain, obs = build_scene("c2")
        q = sample_q(chain, 3, seed=5)[0]
        Tc = rc.arm_camera(0)
    else:
        arm, chain, obs = lc.case(name, tmp_path)
        q = lc.sample(chain, 4, 5)[2]
        Tc = rc.robot_view(arm.scene_model(), q, 1.0)
    sm, dev = arm._scene_device()
    H, W = 36, 48
    intr = rc.intrinsics(H, W)
    qt, Tt = torch.from_numpy(q).cuda(), torch.from_numpy(Tc).cuda()
    cloud = PointCloud(np.zeros((0, 3)), 0.01, bounds=([-4.0, -4.0, -4.0], [4.0, 4.0, 4.0]), capacity=H * W)
    depth, label = arm.depth_images(qt, Tt, W, H, frame="optical", world=False, labels=True)
    assert depth.is_cuda and tuple(depth.shape) == (H, W)
    n_hit = int((label >= 0).sum())
    assert n_hit >= 30, n_hit
    pts, keep = cloud.update_from_depth(depth, intr, Tt, arm=arm, q=qt, padding=0.01)
    assert cloud.count() == 0, f"{name}: {cloud.count()} of {n_hit} rendered pixels survive the arm's own filter"
    depth, label = arm.depth_images(qt, Tt, W, H, frame="optical", labels=True)
    pts, keep = cloud.update_from_depth(depth, intr, Tt, arm=arm, q=qt, padding=0.01)
    keep, lab = keep.cpu().numpy().astype(bool), label.cpu().numpy().reshape(-1)
    assert cloud.count() == keep.sum() and np.all(lab[keep] >= sm.n_rshapes), "only world-labelled pixels survive"
    if name == "c2":
        assert keep.sum() >= 30


def test_render_update_validity_in_one_graph(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    arm, chain, obs = build_scene("c2")
    sm, dev = arm._scene_device()
    H, W = rc.H2, rc.W2
    intr = rc.intrinsics(H, W)
    q0s = sample_q(chain, 3, seed=5)
    cams = [np.ascontiguousarray(rc.arm_camera(k)) for k in range(3)]
    q = sample_q(chain, 64, seed=9)
    box = ([-4.0, -4.0, -4.0], [4.0, 4.0, 4.0])

    def make():
        return PointCloud(np.zeros((0, 3)), 0.01, bounds=box, capacity=H * W)

    def run(cloud, depth, qt0, Tt, qt):
        dev.render_depth(qt0, Tt, intr, H, W, out=depth)
        cloud.update_from_depth(depth[0], intr, Tt, arm=arm, q=qt0[0], padding=0.01)
        return dev.cloud_validity(cloud, qt, 0.02)
    qt = torch.from_numpy(q).cuda()
    eager = []
    for k in range(3):
        depth = torch.empty((1, H, W), dtype=torch.float32, device="cuda")
        m = run(make(), depth, torch.from_numpy(q0s[k:k + 1]).cuda(), torch.from_numpy(cams[k]).cuda(), qt)
        eager.append((m.cpu().numpy().copy(), depth.cpu().numpy().copy()))
        assert (eager[k][1] > 0).sum() >= 30
    assert eager[0][0].any() and len({e[1].tobytes() for e in eager}) == 3
    depth = torch.empty((1, H, W), dtype=torch.float32, device="cuda")
    qt0, Tt = torch.from_numpy(q0s[0:1]).cuda(), torch.from_numpy(cams[0]).cuda()
    cloud = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(cloud, depth, qt0, Tt, qt)               # warm-up outside the capture: the staging tensors are allocated here
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mask = run(cloud, depth, qt0, Tt, qt)
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 2, 0):
        qt0.copy_(torch.from_numpy(q0s[k:k + 1]).cuda())
        Tt.copy_(torch.from_numpy(cams[k]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        _bits(depth.cpu().numpy(), eager[k][1], f"replay {k}: depth")
        _bits(mask.cpu().numpy(), eager[k][0], f"replay {k}: verdicts")


# ---- 7. World.depth_image ----------------------------------------------------------------------------------------------------------------
def test_world_depth_image(fresh_world, torch_cuda):
    arm, chain, obs = build_scene("c2")
    sm, dev = arm._scene_device()
    H, W = rc.H2, rc.W2
    P = rc.numbotics_pose(rc.arm_camera(0))
    far = 6.0
    img = fresh_world.depth_image(W, H, P, far=far)
    assert img.shape == (H, W, 1) and img.dtype == np.float64
    d, l = arm.depth_images(np.asarray(chain.configuration, dtype=np.float64), P, W, H, far=far, labels=True)
    ref = np.where(l >= 0, d.astype(np.float64), far)
    assert (l >= 0).sum() >= 40 and (l == -1).sum() >= 40 and np.all(img[l == -1] == far)
    # the links are world shapes at host-computed poses there and robot shapes at the device's FK here: the same bodies, a few ulps apart
    differ = np.abs(img[:, :, 0] - ref) > 1e-5
    assert differ.sum() <= 2, f"{differ.sum()} pixels differ"
    sharp = fresh_world.depth_image(W, H, P, far=far, bullet_margins=False)
    assert sharp.shape == (H, W, 1)
    # an empty world sees nothing
    from numbotics_amd.physics import World
    assert np.all(World(name="empty").depth_image(5, 4, P) == 1000)
