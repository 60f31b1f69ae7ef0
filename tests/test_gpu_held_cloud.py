"""The held object against point clouds on the device (nbk_held_cloud_*, DeviceModel.held_cloud_validity / held_cloud_clearance /
held_cloud_edge_validity / held_cloud_spline_validity, Arm.in_collision_with_attached(cloud=) / attached_cloud_clearance,
ConnectorParams(attached_sees_cloud=True)): everything bit-equal to the CPU oracle on a model that holds the held shapes as robot
shapes of the holding frame and the cloud's points as sphere world shapes (tests/held_cloud_cases.py).  Needs a real MI355X.

Every mixed case asserts on the REFERENCE, before comparing, that it has rows (edges, trajectories) of both verdicts; the shares of
the fixtures are pinned without a GPU by tests/test_held_cloud_host.py."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd.scenes import build_scene, sample_q
from test_gpu_parity import assert_bitwise, torch_cuda      # noqa: F401  (fixture)
import cloud_cases as cc
import held_cases as hc
import held_cloud_cases as hcc
import held_traj_cases as ht

NT = 8
RES = hcc.RESOLUTION


def _mixed(mask, what):
    assert 0 < int(np.sum(mask)) < len(mask), f"{what}: {int(np.sum(mask))} of {len(mask)} -- not a mixed case"


def _scene(name, margins=True, att=None):
    """-> arm, chain, keep, sm, dev, att, spec, held (DeviceHeld), q (2000, dof), shapes (the robot shapes off the base link, which
    stands on the scanned table), base"""
    arm, chain, obs = build_scene(name, bullet_margins=margins)
    att, b = hc.gripper_box(arm) if att is None else att(arm)
    sm, spec = arm.scene_model(), att.spec(arm)
    dev, held = att._device(arm)
    base = sm.links[sm.rshape_link[0]]._name
    shapes = [k for k in range(sm.n_rshapes) if sm.links[sm.rshape_link[k]]._name != base]
    return types.SimpleNamespace(arm=arm, chain=chain, keep=(obs, b), sm=sm, dev=dev, att=att, spec=spec, held=held,
                                 q=sample_q(chain, 2000, seed=3), shapes=shapes, base=base)


def _cloud(name, **kw):
    from numbotics_amd.physics import PointCloud
    pts, r = hcc.scan(name)
    return PointCloud(pts, r, **kw), pts, r


def _same3(got, ref, what):
    """(valid, end / t_hit, n_samples) against the reference, float bits included."""
    a, b, c = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in got)
    assert np.array_equal(a.astype(bool), ref[0]), f"{what}: valid differs at {np.flatnonzero(a.astype(bool) != ref[0])[:8]}"
    assert_bitwise(b, ref[1], f"{what}: end / t_hit")
    assert c.dtype == np.int32 and np.array_equal(c, ref[2]), f"{what}: n_samples"


# ---- 1. verdicts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c2", "c1"))
@pytest.mark.parametrize("margins", (True, False), ids=("bullet", "sharp"))
def test_verdicts(fresh_world, torch_cuda, name, margins):
    torch = torch_cuda
    x = _scene(name, margins)
    q = x.q[:1000]
    qt = torch.from_numpy(q).cuda()
    for scan in ("dense", "sparse"):
        cloud, pts, r = _cloud(scan)
        for thr in hc.THRESHOLDS:
            ref = hcc.mask(x.sm, x.spec, pts, r, q, thr)
            scene = Oracle(x.sm).validity(q, thr, nthreads=NT) if x.sm.n_pairs else np.zeros(1000, dtype=bool)
            arm_scan = cc.cloud_mask(x.sm, pts, r, q, thr, shapes=x.shapes)
            held = hc.held_mask(x.sm, x.spec, q, thr)
            three = scene | arm_scan | held
            both = three | ref
            # (c1 at thr = 0.01: neighbouring links lie within the threshold of one another, the scene alone rejects every row)
            if not scene.all():
                assert (both & ~three).sum() >= 5, "the held object against the scan must decide rows the three steps let through"
            for B in hcc.BATCHES:
                what = f"{name} {'bullet' if margins else 'sharp'} {scan} thr={thr} B={B}"
                if B >= 63:
                    _mixed(ref[:B], what)
                got = x.dev.held_cloud_validity(x.held, cloud, q[:B], thr)
                assert got.dtype == bool and np.array_equal(got, ref[:B]), f"{what}: bytes differ at {np.flatnonzero(got != ref[:B])[:8]}"
                words = x.dev.held_cloud_validity(x.held, cloud, q[:B], thr, packed=True)
                assert np.array_equal(words, hc.pack_bits(ref[:B])), f"{what}: packed words (the bits beyond B are 0)"
                # accumulate behind the three existing steps: the OR of the four references
                for packed in (False, True):
                    mask = x.dev.validity(qt[:B], thr, packed=packed)
                    x.dev.cloud_validity(cloud, qt[:B], thr, packed=packed, shapes=x.shapes, out=mask)
                    x.dev.held_validity(x.held, qt[:B], thr, packed=packed, out=mask)
                    assert x.dev.held_cloud_validity(x.held, cloud, qt[:B], thr, packed=packed, out=mask) is mask
                    want = hc.pack_bits(both[:B]) if packed else both[:B]
                    assert np.array_equal(mask.cpu().numpy(), want), f"{what}: accumulated {'words' if packed else 'bytes'}"
    # accumulating, the bits beyond B are left as the sibling leaves them: untouched
    cloud, pts, r = _cloud("dense")
    for B in (1, 65):
        ref = hcc.mask(x.sm, x.spec, pts, r, q[:B], 0.0)
        top = np.zeros(((B + 63) // 64,), dtype=np.int64)
        top[-1] = np.iinfo(np.int64).min                         # bit 63 of the last word: beyond B
        ours, theirs = torch.from_numpy(top.copy()).cuda(), torch.from_numpy(top.copy()).cuda()
        x.dev.held_cloud_validity(x.held, cloud, qt[:B], 0.0, packed=True, out=ours)
        x.dev.held_validity(x.held, qt[:B], 0.0, packed=True, out=theirs)
        assert np.array_equal(ours.cpu().numpy(), hc.pack_bits(ref) | top)
        assert np.array_equal(theirs.cpu().numpy(), hc.pack_bits(hc.held_mask(x.sm, x.spec, q[:B], 0.0)) | top)


# ---- 2. held shape kinds and limits ----------------------------------------------------------------------------------------------------
def test_kinds(fresh_world, torch_cuda):
    arm, chain, obs = build_scene("c2")
    q = sample_q(chain, 256, seed=3)
    sm = arm.scene_model()
    clouds = [_cloud(scan) for scan in ("dense", "sparse")]
    for kind, body in hcc.kind_bodies().items():
        att = arm.attach(body, "gripper", pose=hc.trans(0.0, 0.0, hc.BOX_Z))
        spec = att.spec(arm)
        dev, held = att._device(arm)
        for cloud, pts, r in clouds:
            for thr in hc.THRESHOLDS:
                ref = hcc.mask(sm, spec, pts, r, q, thr)
                _mixed(ref, f"{kind} N={len(pts)} thr={thr}")
                got = dev.held_cloud_validity(held, cloud, q, thr)
                assert np.array_equal(got, ref), f"{kind} N={len(pts)} thr={thr}: differs at {np.flatnonzero(got != ref)[:8]}"
            dr, sr, pr = hcc.closest(sm, spec, pts, r, q, 0.3)
            d, s, p = dev.held_cloud_clearance(held, cloud, q, 0.3)
            assert_bitwise(d, dr, f"{kind} N={len(pts)}: clearance")
            assert np.array_equal(s, sr) and np.array_equal(p, pr), f"{kind} N={len(pts)}: clearance indices"
    del obs


def test_eight_shapes(fresh_world, torch_cuda):
    from numbotics_amd.physics.attachment import HeldSpec
    arm, chain, obs = build_scene("c2")
    parts, pose = hcc.eight_parts()
    att = arm.attach(parts, "gripper", pose=pose)
    sm, spec = arm.scene_model(), att.spec(arm)
    dev, held = att._device(arm)
    assert spec.n_shapes == 8
    q = sample_q(chain, 256, seed=3)
    cloud, pts, r = _cloud("dense")
    # at least two different held shapes decide some row: rows that shape h hits and no shape before it
    seen = np.zeros(256, dtype=bool)
    deciders = 0
    for h in range(8):
        one = HeldSpec(frame=spec.frame, A=spec.A, G=spec.G, shape_local=spec.shape_local[h:h + 1], shape_type=spec.shape_type[h:h + 1],
                       shape_param=spec.shape_param[h:h + 1], world_shapes=spec.world_shapes, robot_shapes=spec.robot_shapes)
        m = hcc.mask(sm, one, pts, r, q, 0.0)
        deciders += int((m & ~seen).any())
        seen |= m
    assert deciders >= 2, "at least two different held shapes must decide some row"
    for thr in hc.THRESHOLDS:
        ref = hcc.mask(sm, spec, pts, r, q, thr)
        _mixed(ref, f"H=8 thr={thr}")
        if thr == 0.0:
            assert np.array_equal(ref, seen)
        got = dev.held_cloud_validity(held, cloud, q, thr)
        assert np.array_equal(got, ref), f"H=8 thr={thr}: differs at {np.flatnonzero(got != ref)[:8]}"
    dr, sr, pr = hcc.closest(sm, spec, pts, r, q, 0.3)
    assert len(set(sr[sr >= 0].tolist())) >= 2, "the closest held shape must vary"
    d, s, p = dev.held_cloud_clearance(held, cloud, q, 0.3)
    assert_bitwise(d, dr, "H=8: clearance")
    assert np.array_equal(s, sr) and np.array_equal(p, pr)
    del obs


# ---- 3. grasps ---------------------------------------------------------------------------------------------------------------------
def test_grasps(fresh_world, torch_cuda):
    torch = torch_cuda
    x = _scene("c2")
    cloud, pts, r = _cloud("dense")
    B = 65
    q = x.q[:B]
    ref = hcc.mask(x.sm, x.spec, pts, r, q, 0.0)
    _mixed(ref, "the stored grasp")
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q, 0.0), ref)
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=x.spec.G), ref), "one row: the stored grasp given again"
    rng = np.random.default_rng(1)
    G = np.array([hc.rot_pose(rng) for _ in range(B)])
    one = hcc.mask(x.sm, x.spec, pts, r, q, 0.0, G[0])
    _mixed(one, "one grasp for the call")
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=G[0]), one)
    rows = hcc.mask_rows(x.sm, x.spec, pts, r, q, 0.0, G)
    _mixed(rows, "65 grasps")
    assert (rows != ref).any(), "the grasps change verdicts"
    got = x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=G)
    assert np.array_equal(got, rows), f"a grasp per row: differs at {np.flatnonzero(got != rows)[:8]}"
    Gt = torch.from_numpy(G).cuda()
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, torch.from_numpy(q).cuda(), 0.0, pose=Gt).cpu().numpy(), rows)
    # clearance with a grasp per row, against each row's own model
    d, s, p = x.dev.held_cloud_clearance(x.held, cloud, q, 0.3, pose=G)
    for b in range(0, B, 8):
        dr, sr, pr = hcc.closest(x.sm, x.spec, pts, r, q[b:b + 1], 0.3, G[b])
        assert_bitwise(d[b:b + 1], dr, f"clearance, grasp row {b}")
        assert s[b] == sr[0] and p[b] == pr[0]
    # a NaN in one grasp row hits that row only; a NaN q row hits that row only
    free = np.flatnonzero(~rows)
    bad = G.copy()
    bad[free[0], 1, 2] = np.nan
    bad[free[1], 0, 3] = np.inf
    want = rows.copy(); want[free[:2]] = True
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=bad), want)
    d2, s2, p2 = x.dev.held_cloud_clearance(x.held, cloud, q, 0.3, pose=bad)
    assert np.isnan(d2[free[:2]]).all() and (s2[free[:2]] == -1).all() and (p2[free[:2]] == -1).all()
    keep = np.ones(B, dtype=bool); keep[free[:2]] = False
    assert_bitwise(d2[keep], d[keep], "the other rows")
    qn = q.copy()
    f0 = np.flatnonzero(~ref)
    qn[f0[0], 2] = np.nan
    qn[f0[1], 0] = -np.inf
    want = ref.copy(); want[f0[:2]] = True
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, qn, 0.0), want)
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, qn, 0.0, packed=True), hc.pack_bits(want))
    dn, sn, pn = x.dev.held_cloud_clearance(x.held, cloud, qn, 0.3)
    assert np.isnan(dn[f0[:2]]).all() and (sn[f0[:2]] == -1).all() and (pn[f0[:2]] == -1).all()
    one_bad = x.spec.G.copy(); one_bad[2, 3] = np.nan
    assert x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=one_bad).all()
    with pytest.raises(ValueError):
        x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=G[:7])


# ---- 4. cloud states -----------------------------------------------------------------------------------------------------------------
def test_cloud_states(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    x = _scene("c2")
    q = x.q[:256]
    s, g = hc.edge_set(x.q, 65)
    ctrl, knots = ht.splines(x, 3, S=33)
    pts, r = hcc.scan("dense")
    ref = hcc.mask(x.sm, x.spec, pts, r, q, 0.0)
    dr, sr, pr = hcc.closest(x.sm, x.spec, pts, r, q, 0.3)
    eref = hcc.edges_ref(x.sm, x.spec, pts, r, s, g, hcc.MAXD)
    sref = hcc.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, 3)
    _mixed(ref, "rows"); _mixed(eref[0], "edges"); _mixed(sref[0], "splines")
    # an empty cloud: all free, clearance inf
    empty = PointCloud(np.zeros((0, 3)), 0.01, bounds=([-1, -1, 0], [1, 1, 1]), capacity=8)
    assert not x.dev.held_cloud_validity(x.held, empty, q, 0.0).any()
    d, sh, p = x.dev.held_cloud_clearance(x.held, empty, q, 0.3)
    assert np.isposinf(d).all() and (sh == -1).all() and (p == -1).all()
    assert x.dev.held_cloud_edge_validity(x.held, empty, s, g, RES, hcc.MAXD)[0].all()
    v, th, ns = x.dev.held_cloud_spline_validity(x.held, empty, ctrl, knots, 3, RES)
    assert v.all() and np.isnan(th).all() and np.array_equal(ns, sref[2])
    # the status set by a non-finite point: all hit, clearance NaN, -1, -1; a clean update restores the reference
    cloud = PointCloud(pts, r)
    for bad_value in (np.nan, np.inf):
        bad = pts.copy()
        bad[123, 1] = bad_value
        cloud.update(bad)
        assert cloud.status() == 2
        assert x.dev.held_cloud_validity(x.held, cloud, q, 0.0).all()
        assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q[:65], 0.0, packed=True), hc.pack_bits(np.ones(65, dtype=bool)))
        d, sh, p = x.dev.held_cloud_clearance(x.held, cloud, q, 0.3)
        assert np.isnan(d).all() and (sh == -1).all() and (p == -1).all()
        assert not x.dev.held_cloud_edge_validity(x.held, cloud, s, g, RES, hcc.MAXD)[0].any()
        _same3(x.dev.held_cloud_spline_validity(x.held, cloud, ctrl, knots, 3, RES),
               hcc.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, 3, status=2), "status set: splines")
        cloud.update(pts)
        assert cloud.status() == 0
        assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q, 0.0), ref)
        d, sh, p = x.dev.held_cloud_clearance(x.held, cloud, q, 0.3)
        assert_bitwise(d, dr, "after a clean update")
        assert np.array_equal(sh, sr) and np.array_equal(p, pr)
        _same3(x.dev.held_cloud_edge_validity(x.held, cloud, s, g, RES, hcc.MAXD), eref, "after a clean update: edges")
        _same3(x.dev.held_cloud_spline_validity(x.held, cloud, ctrl, knots, 3, RES), sref, "after a clean update: splines")
    # grids whose box does not contain the held object (the points are filed in border cells), and other cells: still bit-equal
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    half = (lo, np.array([hi[0], 0.5 * (lo[1] + hi[1]), hi[2]]))
    for what, kw in (("box elsewhere", dict(bounds=([5, 5, 5], [6, 6, 6]), cell=0.1)), ("half box", dict(bounds=half)),
                     ("one cell", dict(cell=10.0)), ("cell 0.02", dict(cell=0.02))):
        c = PointCloud(pts, r, **kw)
        assert np.array_equal(x.dev.held_cloud_validity(x.held, c, q, 0.0), ref), what
        d, sh, p = x.dev.held_cloud_clearance(x.held, c, q, 0.3)
        assert_bitwise(d, dr, what)
        assert np.array_equal(sh, sr) and np.array_equal(p, pr), what
        _same3(x.dev.held_cloud_edge_validity(x.held, c, s, g, RES, hcc.MAXD), eref, f"{what}: edges")


# ---- 5. clearance --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", ("dense", "sparse"))
def test_clearance(fresh_world, torch_cuda, scan):
    torch = torch_cuda
    x = _scene("c2")
    cloud, pts, r = _cloud(scan)
    for d_max in (0.05, 0.3):
        dr, sr, pr = hcc.closest(x.sm, x.spec, pts, r, x.q[:1000], d_max)
        fin = np.isfinite(dr)
        assert fin.sum() >= 100 and (~fin).sum() >= 100, "rows within d_max and rows beyond it"
        assert (dr < 0).sum() >= 20, "negative distances: the box, margin included, reaches into the points' spheres"
        assert (dr[fin] > 0).any() and (sr[fin] == 0).all() and (sr[~fin] == -1).all()
        for B in hcc.BATCHES:
            d, s, p = x.dev.held_cloud_clearance(x.held, cloud, x.q[:B], d_max)
            assert_bitwise(d, dr[:B], f"{scan} d_max={d_max} B={B}: distance")
            assert s.dtype == np.int32 and np.array_equal(s, sr[:B]) and p.dtype == np.int32 and np.array_equal(p, pr[:B]), \
                f"{scan} d_max={d_max} B={B}: indices"
    dt, st, pt = x.dev.held_cloud_clearance(x.held, cloud, torch.from_numpy(x.q[:1000]).cuda(), 0.3)
    assert dt.is_cuda and st.dtype == torch.int32
    assert_bitwise(dt.cpu().numpy(), dr, "device tensors in, device tensors out")
    # the public entry
    d1, s1, p1 = x.arm.attached_cloud_clearance(x.q[:64], x.att, cloud, 0.3)
    assert_bitwise(d1, dr[:64], "attached_cloud_clearance")
    assert np.array_equal(s1, sr[:64]) and np.array_equal(p1, pr[:64])
    near, far = int(np.flatnonzero(fin)[0]), int(np.flatnonzero(~fin)[0])
    out = x.arm.attached_cloud_clearance(x.q[near], x.att, cloud, 0.3)
    assert isinstance(out[0], float) and out == (float(dr[near]), 0, int(pr[near]))
    assert x.arm.attached_cloud_clearance(x.q[far], x.att, cloud, 0.3) == (np.inf, -1, -1)


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", ("dense", "sparse"))
def test_edges(fresh_world, torch_cuda, scan):
    torch = torch_cuda
    x = _scene("c2")
    cloud, pts, r = _cloud(scan)
    s, g = hc.edge_set(x.q, hcc.N_EDGES)
    g[7] = s[7]                                                  # a degenerate edge
    s[11, 3] = np.nan                                            # an edge with a NaN start
    given = 1.1 * np.linalg.norm(g - s, axis=1)
    both_m = hc.held_model(x.sm, x.spec, keep_scene=True)
    for mode, maxd, thr, dist in (("connect", hcc.MAXD, 0.0, None), ("steer", hcc.MAXD_STEER, 0.01, None), ("connect", hcc.MAXD, -0.002, given)):
        ref = hcc.edges_ref(x.sm, x.spec, pts, r, s, g, maxd, mode, thr, dist)
        assert not ref[0][7] and ref[2][7] == 0 and np.isnan(ref[1][7]).all() and not ref[0][11]
        for E in hcc.EDGE_COUNTS:
            if E >= 63:
                _mixed(ref[0][:E], f"{scan} {mode} E={E}")
            got = x.dev.held_cloud_edge_validity(x.held, cloud, s[:E], g[:E], RES, maxd, mode=mode, threshold=thr,
                                                 dist=None if dist is None else dist[:E])
            assert got[0].dtype == bool
            _same3(got, tuple(a[:E] for a in ref), f"{scan} {mode} thr={thr} E={E}")
        # out= behind the three existing steps: the AND of the four references
        three = (Oracle(both_m).edge_validity(s, g, RES, maxd, mode=mode, threshold=thr, dist=dist, nthreads=NT)[0]
                 & hcc.arm_cloud_edges_ref(x.sm, pts, r, s, g, maxd, mode, thr, dist, shapes=x.shapes)[0])
        want = three & ref[0]
        assert (three & ~want).sum() >= 3 and want.sum() >= 3, "the held object against the scan must block edges the three steps let through"
        st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
        dt = None if dist is None else torch.from_numpy(dist).cuda()
        kw = dict(mode=mode, threshold=thr, dist=dt)
        res = x.dev.edge_validity(st, gt, RES, maxd, **kw)
        x.dev.cloud_edge_validity(cloud, st, gt, RES, maxd, shapes=x.shapes, out=res[0], **kw)
        x.dev.held_edge_validity(x.held, st, gt, RES, maxd, out=res[0], **kw)
        assert np.array_equal(res[0].cpu().numpy().astype(bool), three), f"{scan} {mode}: the three steps"
        out = x.dev.held_cloud_edge_validity(x.held, cloud, st, gt, RES, maxd, out=res[0], **kw)
        assert out[0] is res[0]
        _same3((res[0], out[1], out[2]), (want, ref[1], ref[2]), f"{scan} {mode}: accumulated")
    # another grasp for the call; a non-finite one invalidates every edge
    G = hc.rot_pose(np.random.default_rng(4))
    ref = hcc.edges_ref(x.sm, x.spec, pts, r, s, g, hcc.MAXD, G=G)
    _mixed(ref[0], "edges, another grasp")
    _same3(x.dev.held_cloud_edge_validity(x.held, cloud, s, g, RES, hcc.MAXD, pose=G), ref, "edges, another grasp")
    bad = G.copy(); bad[0, 0] = np.nan
    assert not x.dev.held_cloud_edge_validity(x.held, cloud, s, g, RES, hcc.MAXD, pose=bad)[0].any()


# ---- 7. splines ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", (1, 3, 5))
def test_splines(fresh_world, torch_cuda, degree):
    torch = torch_cuda
    from spline_ref import reference_splines
    from cloud_spline_ref import merge_scene_and_cloud
    x = _scene("c2")
    ctrl, knots = ht.splines(x, degree)
    for scan in ("dense", "sparse"):
        cloud, pts, r = _cloud(scan)
        for thr in (0.0, 0.01):
            ref = hcc.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, degree, thr)
            _mixed(ref[0], f"degree {degree} {scan} thr={thr}")
            _mixed(ref[0][:64], f"degree {degree} {scan} thr={thr} S=64")
            for S in ht.SPLINE_COUNTS:
                got = x.dev.held_cloud_spline_validity(x.held, cloud, ctrl[:S], knots, degree, RES, threshold=thr)
                assert got[0].dtype == bool
                _same3(got, tuple(a[:S] for a in ref), f"degree {degree} {scan} thr={thr} S={S}")
        # accumulated into the scene's result
        ref = hcc.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, degree)
        scene = reference_splines(Oracle(x.sm), ctrl, knots, degree, RES, 0.0)
        want = merge_scene_and_cloud(scene, ref)
        assert (scene[0] & ~want[0]).sum() >= 1 and want[0].any()
        ct = torch.from_numpy(ctrl).cuda()
        out = x.dev.spline_validity(ct, knots, degree, RES)
        got = x.dev.held_cloud_spline_validity(x.held, cloud, ct, knots, degree, RES, out=out)
        assert all(a is b for a, b in zip(got, out))
        _same3(got, want, f"degree {degree} {scan}: accumulated")
    if degree == 3:
        cloud, pts, r = _cloud("dense")
        G = hc.rot_pose(np.random.default_rng(4))
        ref = hcc.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, 3, G=G)
        _mixed(ref[0], "splines, another grasp")
        _same3(x.dev.held_cloud_spline_validity(x.held, cloud, ctrl, knots, 3, RES, pose=G), ref, "splines, another grasp")
        bad = G.copy(); bad[0, 0] = np.nan
        valid, t_hit, ns = x.dev.held_cloud_spline_validity(x.held, cloud, ctrl, knots, 3, RES, pose=bad)
        assert not valid.any() and (t_hit == 0.0).all() and np.array_equal(ns, ref[2])
        valid, t_hit, ns = x.dev.held_cloud_spline_validity(x.held, cloud, ctrl, knots[::-1].copy(), 3, RES)
        assert not valid.any() and np.isnan(t_hit).all() and (ns == 0).all()


# ---- 8. the public layer ---------------------------------------------------------------------------------------------------------------
def test_arm_entries(fresh_world, torch_cuda):
    torch = torch_cuda
    x = _scene("c2")
    cloud, pts, r = _cloud("dense")
    q = x.q[:256]
    for thr in (0.0, 0.01):
        alone, scan = hc.held_mask(x.sm, x.spec, q, thr), hcc.mask(x.sm, x.spec, pts, r, q, thr)
        assert (scan & ~alone).sum() >= 5 and (alone & ~scan).sum() >= 1
        assert np.array_equal(x.arm.in_collision_with_attached(q, x.att, thr), alone), "cloud=None keeps today's result"
        assert np.array_equal(x.arm.in_collision_with_attached(q, x.att, thr, cloud=cloud), alone | scan)
    want = hc.held_mask(x.sm, x.spec, q[:6], 0.0) | hcc.mask(x.sm, x.spec, pts, r, q[:6], 0.0)
    hit = x.arm.in_collision_with_attached(q[:6].reshape(2, 3, -1), x.att, cloud=cloud)
    assert hit.shape == (2, 3) and np.array_equal(hit.reshape(-1), want)
    both = alone | scan
    for b in np.concatenate((np.flatnonzero(scan & ~alone)[:3], np.flatnonzero(~both)[:3])):
        assert x.arm.in_collision_with_attached(q[b], x.att, 0.01, cloud=cloud) is bool(both[b])
        assert x.arm.in_collision_with_attached(q[b], x.att, 0.01) is bool(alone[b])
    got = x.arm.in_collision_with_attached(torch.from_numpy(q).cuda(), x.att, 0.01, cloud=cloud)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), both)
    G = hc.rot_pose(np.random.default_rng(4))
    want = hc.held_mask(x.sm, x.spec, q, 0.0, G=G) | hcc.mask(x.sm, x.spec, pts, r, q, 0.0, G)
    assert np.array_equal(x.arm.in_collision_with_attached(q, x.att, 0.0, pose=G, cloud=cloud), want)


def test_connector(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, DiscreteConnector
    from spline_ref import reference_splines
    from cloud_spline_ref import reference_cloud_splines, merge_scene_and_cloud
    x = _scene("c2")
    pts, r = hcc.scan("sparse")
    cloud = PointCloud(pts, r)
    s, g = hc.edge_set(x.q, hcc.N_EDGES)
    kw = dict(arm=x.arm, cloud=cloud, cloud_ignore_links=(x.base,), attached=x.att, resolution=RES, max_distance=hcc.MAXD_STEER)
    con = DiscreteConnector(ConnectorParams(attached_sees_cloud=True, **kw))
    blind = DiscreteConnector(ConnectorParams(**kw))
    both_m = hc.held_model(x.sm, x.spec, keep_scene=True)
    three, four = {}, {}
    for m in ("connect", "steer"):
        a = Oracle(both_m).edge_validity(s, g, RES, hcc.MAXD_STEER, mode=m, nthreads=NT)
        b = hcc.arm_cloud_edges_ref(x.sm, pts, r, s, g, hcc.MAXD_STEER, m, shapes=x.shapes)
        c = hcc.edges_ref(x.sm, x.spec, pts, r, s, g, hcc.MAXD_STEER, m)
        three[m] = (a[0] & b[0], a[1])
        four[m] = (three[m][0] & c[0], a[1])
        _mixed(four[m][0], f"connector {m}")
        assert (three[m][0] & ~four[m][0]).sum() >= 3, "the flag must reject edges the three steps accept"
    ok = con.connect_batch(s, g)
    assert ok.dtype == bool and np.array_equal(ok, four["connect"][0])
    ok, end = con.steer_batch(s, g)
    assert np.array_equal(ok, four["steer"][0])
    assert_bitwise(end, four["steer"][1], "steer end states")
    # without the flag: today's three-step result on the same edges
    old = blind.connect_batch(s, g)
    assert np.array_equal(old, three["connect"][0]) and (old != con.connect_batch(s, g)).sum() >= 3
    ok3, end3 = blind.steer_batch(s, g)
    assert np.array_equal(ok3, three["steer"][0])
    assert_bitwise(end3, three["steer"][1], "steer end states, without the flag")
    ref = four["connect"][0]
    for e in np.concatenate((np.flatnonzero(ref)[:3], np.flatnonzero(three["connect"][0] & ~ref)[:3])):
        out = con.connect(s[e], g[e])
        assert (out is not None) == bool(ref[e]), f"connect, edge {e}"
        assert (blind.connect(s[e], g[e]) is not None) == bool(three["connect"][0][e]), f"connect without the flag, edge {e}"
        out = con.steer(s[e], g[e])
        assert (out is not None) == bool(four["steer"][0][e]), f"steer, edge {e}"
        if out is not None:
            assert_bitwise(out, four["steer"][1][e], "steer returns traj(T_f)")
    q = x.q[:32]
    hit3 = Oracle(both_m).validity(q, 0.0) | cc.cloud_mask(x.sm, pts, r, q, 0.0, shapes=x.shapes)
    hit4 = hit3 | hcc.mask(x.sm, x.spec, pts, r, q, 0.0)
    assert (hit4 & ~hit3).any()
    assert np.array_equal(np.array([con.is_valid(q[b]) for b in range(32)]), ~hit4)
    assert np.array_equal(np.array([blind.is_valid(q[b]) for b in range(32)]), ~hit3)
    # smoothed trajectories
    ctrl, knots = ht.splines(x, 3)
    t3 = merge_scene_and_cloud(reference_splines(Oracle(both_m), ctrl, knots, 3, RES, 0.0),
                               reference_cloud_splines(x.sm, pts, r, ctrl, knots, 3, RES, 0.0, shapes=x.shapes))
    t4 = merge_scene_and_cloud(t3, hcc.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, 3))
    _mixed(t4[0], "connector, trajectories")
    assert (t3[0] & ~t4[0]).sum() >= 1, "the flag must reject a trajectory the three steps accept"
    _same3(con.validate_trajectories(ctrl, degree=3, cloud=cloud, attached=x.att), t4, "validate_trajectories with the flag")
    _same3(blind.validate_trajectories(ctrl, degree=3, cloud=cloud, attached=x.att), t3, "validate_trajectories without the flag")


# ---- 9. capture ----------------------------------------------------------------------------------------------------------------------
def test_capture(fresh_world, torch_cuda):
    """validity -> cloud_validity -> held_validity -> held_cloud_validity(out=) and the edge chain in captured graphs; replays follow
    the cloud's update, q and the grasp tensor rewritten in place.  A call that allocated or synchronised inside the capture would
    end it with an error."""
    torch = torch_cuda
    from numbotics_amd.physics import PointCloud
    x = _scene("c2")
    B, E = 256, 65
    rng = np.random.default_rng(9)
    qs = [x.q[k * B:(k + 1) * B] for k in range(3)]
    Gs = [hc.rot_pose(rng) for _ in range(3)]
    clouds = [np.ascontiguousarray(cc.scan(1000, seed=k)) for k in range(3)]
    r = 0.01
    cloud = PointCloud(clouds[0], r, bounds=([-0.6, -0.6, 0.0], [0.6, 0.6, 1.0]))
    qt = torch.from_numpy(qs[0].copy()).cuda()
    Gt = torch.from_numpy(Gs[0].copy()).cuda()
    delta = rng.uniform(-0.5, 0.5, (E, x.chain.dof))
    st, gt = torch.from_numpy(qs[0][:E].copy()).cuda(), torch.from_numpy(qs[0][:E] + delta).cuda()
    ws = [torch.empty((n,), dtype=torch.uint8, device="cuda") for n in
          (x.dev.cloud_edge_workspace_bytes(E), x.dev.held_edge_workspace_bytes(E), x.dev.held_cloud_edge_workspace_bytes(E))]

    def rows():
        mask = x.dev.validity(qt, 0.0)
        x.dev.cloud_validity(cloud, qt, 0.0, shapes=x.shapes, out=mask)
        x.dev.held_validity(x.held, qt, 0.0, pose=Gt, out=mask)
        x.dev.held_cloud_validity(x.held, cloud, qt, 0.0, pose=Gt, out=mask)
        return mask

    def edges():
        valid, end, ns = x.dev.edge_validity(st, gt, RES, hcc.MAXD)
        x.dev.cloud_edge_validity(cloud, st, gt, RES, hcc.MAXD, shapes=x.shapes, out=valid, workspace=ws[0])
        x.dev.held_edge_validity(x.held, st, gt, RES, hcc.MAXD, pose=Gt, out=valid, workspace=ws[1])
        x.dev.held_cloud_edge_validity(x.held, cloud, st, gt, RES, hcc.MAXD, pose=Gt, out=valid, workspace=ws[2])
        return valid

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rows(); edges()                                          # warm-up outside the capture
        side.synchronize()
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, stream=side):
            mask = rows()
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=side):
            valid = edges()
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for k in (1, 2):
        cloud.update(clouds[k])
        qt.copy_(torch.from_numpy(qs[k].copy()).cuda())
        Gt.copy_(torch.from_numpy(Gs[k].copy()).cuda())
        st.copy_(torch.from_numpy(qs[k][:E].copy()).cuda())
        gt.copy_(torch.from_numpy(qs[k][:E] + delta).cuda())
        g1.replay(); g2.replay()
        torch.cuda.synchronize()
        both_m = hc.held_model(x.sm, x.spec, Gs[k], keep_scene=True)
        own = hcc.mask(x.sm, x.spec, clouds[k], r, qs[k], 0.0, Gs[k])
        three = Oracle(both_m).validity(qs[k], 0.0, nthreads=NT) | cc.cloud_mask(x.sm, clouds[k], r, qs[k], 0.0, shapes=x.shapes)
        ref = three | own
        _mixed(ref, f"replay {k}")
        assert (ref & ~three).any(), f"replay {k}: the new step decides rows"
        assert np.array_equal(mask.cpu().numpy().astype(bool), ref), f"replay {k}: rows"
        assert np.array_equal(rows().cpu().numpy().astype(bool), ref), f"replay {k}: the eager chain"
        s, g = qs[k][:E], gt.cpu().numpy()
        eown = hcc.edges_ref(x.sm, x.spec, clouds[k], r, s, g, hcc.MAXD, G=Gs[k])[0]
        ethree = (Oracle(both_m).edge_validity(s, g, RES, hcc.MAXD, nthreads=NT)[0]
                  & hcc.arm_cloud_edges_ref(x.sm, clouds[k], r, s, g, hcc.MAXD, shapes=x.shapes)[0])
        eref = ethree & eown
        _mixed(eref, f"replay {k}: edges")
        assert np.array_equal(valid.cpu().numpy().astype(bool), eref), f"replay {k}: edges"
        seen.append(own.tobytes())
    assert seen[0] != seen[1]
