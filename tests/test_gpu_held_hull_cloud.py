"""Held meshes against point clouds on the device: a hull attachment that has opted in (``Arm.attach(..., meshes=True,
mesh_scans=True)``, ``DeviceHeld(..., scans=True)``, nbk_held_set_cloud_hulls) through all seven held-versus-cloud entries and the
public layer on top of them, everything bit-equal to the CPU oracle on the combined descriptor -- the scene's with the held shapes as
robot shapes S + h and the held hulls appended to its hull tables -- with the cloud's points as sphere world shapes
(tests/held_hull_cloud_cases.py).  Needs a real MI355X.

What the fixtures must have for these comparisons to mean something (mixed verdicts, rows a hull decides and rows a primitive decides,
a hull closest, a point inside a hull, FREE / COLLISION / cap exits) is pinned on the reference, without a GPU, by
tests/test_held_hull_cloud_host.py; the mixed cases assert it once more here, on the reference, before comparing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from test_gpu_parity import assert_bitwise, torch_cuda      # noqa: F401  (fixture)
from ca_ref import FREE, COLLISION
import held_cases as hc
import held_cloud_cases as hcc
import held_hull_cases as hh
import held_hull_cloud_cases as hk
import held_records_cases as hr

RES = hk.RESOLUTION
MAXD = hk.MAXD
MSG = "held meshes do not see scans yet"
ALL_THR = hk.THRESHOLDS + (hk.DEEP,)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _mixed(mask, what):
    assert 0 < int(np.sum(mask)) < len(mask), f"{what}: {int(np.sum(mask))} of {len(mask)} -- not a mixed case"


def _x(name, kind, scans=True):
    x = hk.scene(name, kind, scans)
    x.dev, x.held = hk.device(x, scans)
    return x


def _cloud(name, **kw):
    from numbotics_amd.physics import PointCloud
    pts, r = hcc.scan(name)
    return PointCloud(pts, r, **kw), pts, r


def _same3(got, ref, what):
    """(valid, end / t_hit, n_samples) of a sampled call against the reference, float bits included."""
    a, b, c = (_np(v) for v in got)
    assert np.array_equal(a.astype(bool), ref[0]), f"{what}: valid differs at {np.flatnonzero(a.astype(bool) != ref[0])[:8]}"
    assert_bitwise(b, ref[1], f"{what}: end / t_hit")
    assert c.dtype == np.int32 and np.array_equal(c, ref[2]), f"{what}: n_samples"


def _same_ca(got, ref, what):
    """(valid, ..., t_free, status) of a certified call against (valid, ..., t_free, status) of the reference."""
    v, t, st = _np(got[0]), _np(got[-2]), _np(got[-1])
    assert np.array_equal(v.astype(bool), ref[0]), f"{what}: valid differs at {np.flatnonzero(v.astype(bool) != ref[0])[:8]}"
    assert_bitwise(t, ref[-2], f"{what}: t_free")
    assert st.dtype == np.int32 and np.array_equal(st, ref[-1]), f"{what}: status differs at {np.flatnonzero(st != ref[-1])[:8]}"


# ---- 1. verdicts and clearance -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("c2", k) for k in hk.FIXTURES] + [("c5m", "rock")])
def test_verdicts_and_clearance(fresh_world, torch_cuda, name, kind):
    torch = torch_cuda
    x = _x(name, kind)
    q = x.q[:hk.N_ROWS]
    qt = torch.from_numpy(q).cuda()
    for scan in hcc.SCANS:
        cloud, pts, r = _cloud(scan)
        for thr in ALL_THR:
            ref = hk.mask(x.sm, x.spec, pts, r, q, thr)
            flat_deep = kind == "flat" and thr == hk.DEEP             # (a flat hull has no inside: all free there)
            for B in hk.BATCHES:
                what = f"{name} {kind} {scan} thr={thr} B={B}"
                if B >= 63 and not flat_deep and (thr != hk.DEEP or scan == "dense"):
                    _mixed(ref[:B], what)
                got = x.dev.held_cloud_validity(x.held, cloud, q[:B], thr)
                assert got.dtype == bool and np.array_equal(got, ref[:B]), f"{what}: bytes differ at {np.flatnonzero(got != ref[:B])[:8]}"
                words = x.dev.held_cloud_validity(x.held, cloud, q[:B], thr, packed=True)
                assert np.array_equal(words, hc.pack_bits(ref[:B])), f"{what}: packed words (the bits beyond B are 0)"
            # accumulate into a mask that holds the scene's verdicts and the held object's against the scene
            scene = Oracle(x.sm).validity(q, thr, nthreads=8) | hh.held_mask(x.sm, x.spec, q, thr)
            for packed in (False, True):
                mask = x.dev.validity(qt, thr, packed=packed)
                x.dev.held_validity(x.held, qt, thr, packed=packed, out=mask)
                assert x.dev.held_cloud_validity(x.held, cloud, qt, thr, packed=packed, out=mask) is mask
                want = hc.pack_bits(scene | ref) if packed else scene | ref
                assert np.array_equal(_np(mask), want), f"{name} {kind} {scan} thr={thr}: accumulated {'words' if packed else 'bytes'}"
            if thr == 0.0:
                assert (ref & ~scene).sum() >= 3, "the held object against the scan decides rows the scene lets through"
        dr, sr, pr = hk.closest(x.sm, x.spec, pts, r, q, hk.D_MAX)
        for B in hk.BATCHES:
            d, s, p = x.dev.held_cloud_clearance(x.held, cloud, q[:B], hk.D_MAX)
            assert_bitwise(d, dr[:B], f"{name} {kind} {scan} B={B}: clearance")
            assert s.dtype == np.int32 and np.array_equal(s, sr[:B]) and p.dtype == np.int32 and np.array_equal(p, pr[:B]), \
                f"{name} {kind} {scan} B={B}: clearance indices"


# ---- 2. grasps, non-finite rows ---------------------------------------------------------------------------------------------------------
def test_grasps_and_bad_rows(fresh_world, torch_cuda):
    torch = torch_cuda
    x = _x("c2", "mixed")
    cloud, pts, r = _cloud("dense")
    B = 65
    q = x.q[:B]
    ref = hk.mask(x.sm, x.spec, pts, r, q, 0.0)
    _mixed(ref, "the stored grasp")
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q, 0.0), ref)
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=x.spec.G), ref), "one row: the stored grasp given again"
    rng = np.random.default_rng(1)
    G = np.array([x.spec.G @ hc.rot_pose(rng, 0.4, 0.03) @ hc.trans(0, 0, -hc.BOX_Z) for _ in range(B)])
    one = hk.mask(x.sm, x.spec, pts, r, q, 0.0, G[0])
    _mixed(one, "one grasp for the call")
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=G[0]), one)
    rows = hk.mask_rows(x.sm, x.spec, pts, r, q, 0.0, G)
    _mixed(rows, "65 grasps")
    assert (rows != ref).any(), "the grasps change verdicts"
    got = x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=G)
    assert np.array_equal(got, rows), f"a grasp per row: differs at {np.flatnonzero(got != rows)[:8]}"
    Gt = torch.from_numpy(G).cuda()
    assert np.array_equal(_np(x.dev.held_cloud_validity(x.held, cloud, torch.from_numpy(q).cuda(), 0.0, pose=Gt)), rows)
    # clearance and records with one grasp and with a grasp per row, each row against its own model
    d1, s1, p1 = x.dev.held_cloud_clearance(x.held, cloud, q, hk.D_MAX, pose=G[0])
    dr, sr, pr = hk.closest(x.sm, x.spec, pts, r, q, hk.D_MAX, G[0])
    assert_bitwise(d1, dr, "clearance, one grasp")
    assert np.array_equal(s1, sr) and np.array_equal(p1, pr)
    d, s, p = x.dev.held_cloud_clearance(x.held, cloud, q, hk.D_MAX, pose=G)
    rec = x.dev.held_cloud_records(x.held, cloud, q, hk.D_MAX, pose=G)
    for b in range(0, B, 8):
        raw = hk.records_raw(x, pts, r, q[b:b + 1], G[b])
        want = hk.records_ref(x, raw, hk.D_MAX, False)
        assert_bitwise(d[b:b + 1], want[0], f"clearance, grasp row {b}")
        assert s[b] == want[1][0] and p[b] == want[2][0]
        hr.assert_cloud_records(tuple(f[b:b + 1] for f in rec), want, f"records, grasp row {b}")
    # a NaN in one grasp row hits that row only; a NaN q row hits that row only
    free = np.flatnonzero(~rows)
    bad = G.copy()
    bad[free[0], 1, 2] = np.nan
    bad[free[1], 0, 3] = np.inf
    want = rows.copy(); want[free[:2]] = True
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=bad), want)
    d2, s2, p2 = x.dev.held_cloud_clearance(x.held, cloud, q, hk.D_MAX, pose=bad)
    assert np.isnan(d2[free[:2]]).all() and (s2[free[:2]] == -1).all() and (p2[free[:2]] == -1).all()
    keep = np.ones(B, dtype=bool); keep[free[:2]] = False
    assert_bitwise(d2[keep], d[keep], "the other rows")
    rec2 = x.dev.held_cloud_records(x.held, cloud, q, hk.D_MAX, pose=bad)
    assert all(np.isnan(_np(rec2[k])[free[:2]]).all() for k in (0, 3, 4))
    qn = q.copy()
    f0 = np.flatnonzero(~ref)
    qn[f0[0], 2] = np.nan
    qn[f0[1], 0] = -np.inf
    want = ref.copy(); want[f0[:2]] = True
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, qn, 0.0), want)
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, qn, 0.0, packed=True), hc.pack_bits(want))
    dn, sn, pn = x.dev.held_cloud_clearance(x.held, cloud, qn, hk.D_MAX)
    assert np.isnan(dn[f0[:2]]).all() and (sn[f0[:2]] == -1).all() and (pn[f0[:2]] == -1).all()
    recn = x.dev.held_cloud_records(x.held, cloud, qn, hk.D_MAX, per_shape=True)
    assert all(np.isnan(_np(recn[k])[f0[:2]]).all() for k in (0, 3, 4))
    one_bad = x.spec.G.copy(); one_bad[2, 3] = np.nan
    assert x.dev.held_cloud_validity(x.held, cloud, q, 0.0, pose=one_bad).all()


# ---- 3. records ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("rock", "flat", "mixed", "eight"))
def test_records(fresh_world, torch_cuda, kind):
    x = _x("c2", kind)
    q = x.q[:130]
    for scan in hcc.SCANS:
        cloud, pts, r = _cloud(scan)
        raw = hk.records_raw(x, pts, r, q)
        for per_shape in (False, True):
            ref = hk.records_ref(x, raw, hk.D_MAX, per_shape)
            win = ref[1] >= 0
            assert win.any() and not win.all(), "some records win, some are beyond d_max"
            assert (ref[0][win] < 0).any(), "a winner inside the shape: the EPA pass"
            for B in (1, 63, 64, 65, 130):
                got = x.dev.held_cloud_records(x.held, cloud, q[:B], hk.D_MAX, per_shape=per_shape)
                hr.assert_cloud_records(got, ref, f"{kind} {scan} per_shape={per_shape} B={B}", B)
            got = x.dev.held_cloud_records(x.held, cloud, q, hk.D_MAX, per_shape=per_shape, witness=False, jacobian=False)
            assert got[3] is None and got[4] is None
            hr.assert_cloud_records(got, ref, f"{kind} {scan} per_shape={per_shape}: the winner alone")


# ---- 4. sampled edges and splines ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("rock", "mixed", "eight"))
def test_sampled_edges(fresh_world, torch_cuda, kind):
    torch = torch_cuda
    x = _x("c2", kind)
    s, g = hk.edges(x)
    g[7] = s[7]                                                  # a degenerate edge
    s[11, 3] = np.nan                                            # an edge with a NaN start
    given = 1.1 * np.linalg.norm(g - s, axis=1)
    G = x.spec.G @ hc.rot_pose(np.random.default_rng(4), 0.4, 0.03) @ hc.trans(0, 0, -hc.BOX_Z)
    for scan in hcc.SCANS:
        cloud, pts, r = _cloud(scan)
        for mode, maxd, thr, dist in (("connect", MAXD, 0.0, None), ("steer", hcc.MAXD_STEER, 0.01, None), ("connect", MAXD, -0.002, given),
                                      ("connect", MAXD, hk.DEEP, None)):
            ref = hk.edges_ref(x.sm, x.spec, pts, r, s, g, maxd, mode, thr, dist)
            assert not ref[0][7] and ref[2][7] == 0 and not ref[0][11]
            for E in hk.EDGE_COUNTS:
                if E >= 63:
                    _mixed(ref[0][:E], f"{kind} {scan} {mode} thr={thr} E={E}")
                got = x.dev.held_cloud_edge_validity(x.held, cloud, s[:E], g[:E], RES, maxd, mode=mode, threshold=thr,
                                                     dist=None if dist is None else dist[:E])
                assert got[0].dtype == bool
                _same3(got, tuple(a[:E] for a in ref), f"{kind} {scan} {mode} thr={thr} E={E}")
        # accumulated into the scene's result; one grasp tensor for the call
        ref = hk.edges_ref(x.sm, x.spec, pts, r, s, g, G=G)
        _mixed(ref[0], "edges, another grasp")
        scene = Oracle(x.sm).edge_validity(s, g, RES, MAXD, nthreads=8)
        assert (scene[0] & ~ref[0]).sum() >= 3
        st, gt, Gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(G).cuda()
        res = x.dev.edge_validity(st, gt, RES, MAXD)
        out = x.dev.held_cloud_edge_validity(x.held, cloud, st, gt, RES, MAXD, pose=Gt, out=res[0])
        assert out[0] is res[0]
        _same3((res[0], out[1], out[2]), (scene[0] & ref[0], ref[1], ref[2]), f"{kind} {scan}: accumulated, a grasp tensor")
        bad = G.copy(); bad[0, 0] = np.nan
        assert not x.dev.held_cloud_edge_validity(x.held, cloud, s, g, RES, MAXD, pose=bad)[0].any()


@pytest.mark.parametrize("degree", (1, 3, 5))
def test_sampled_splines(fresh_world, torch_cuda, degree):
    torch = torch_cuda
    from spline_ref import reference_splines
    from cloud_spline_ref import merge_scene_and_cloud
    G = None
    for kind in ("mixed", "eight"):
        x = _x("c2", kind)
        ctrl, knots = hk.splines(x, degree)
        for scan in hcc.SCANS:
            cloud, pts, r = _cloud(scan)
            for thr in (0.0, 0.01, hk.DEEP):
                ref = hk.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, degree, thr)
                _mixed(ref[0], f"{kind} degree {degree} {scan} thr={thr}")
                _mixed(ref[0][:64], f"{kind} degree {degree} {scan} thr={thr} S=64")
                for S in hk.SPLINE_COUNTS:
                    got = x.dev.held_cloud_spline_validity(x.held, cloud, ctrl[:S], knots, degree, RES, threshold=thr)
                    assert got[0].dtype == bool
                    _same3(got, tuple(a[:S] for a in ref), f"{kind} degree {degree} {scan} thr={thr} S={S}")
            # accumulated into the scene's result, with one grasp tensor
            G = x.spec.G @ hc.rot_pose(np.random.default_rng(4), 0.4, 0.03) @ hc.trans(0, 0, -hc.BOX_Z)
            ref = hk.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, degree, G=G)
            _mixed(ref[0], f"{kind} degree {degree} {scan}: another grasp")
            scene = reference_splines(Oracle(x.sm), ctrl, knots, degree, RES, 0.0)
            want = merge_scene_and_cloud(scene, ref)
            ct = torch.from_numpy(ctrl).cuda()
            out = x.dev.spline_validity(ct, knots, degree, RES)
            got = x.dev.held_cloud_spline_validity(x.held, cloud, ct, knots, degree, RES, pose=torch.from_numpy(G).cuda(), out=out)
            assert all(a is b for a, b in zip(got, out))
            _same3(got, want, f"{kind} degree {degree} {scan}: accumulated, a grasp tensor")


# ---- 5. certified edges and splines -----------------------------------------------------------------------------------------------------
def _scene_items(x, s, g, maxd, mode, thr):
    from continuous_ref import reference_continuous, edge_span
    a = reference_continuous(x.sm, Oracle(x.sm), s, g, maxd, mode=mode, threshold=thr, max_iter=hk.MAX_ITER, slack=1e-6)
    spans = [edge_span(s[e], g[e], None, maxd, mode) for e in range(s.shape[0])]
    live = np.array([sp is not None for sp in spans], dtype=bool)
    Tf = np.array([sp[1] if sp is not None else np.nan for sp in spans])
    return a, Tf, live


@pytest.mark.parametrize("kind", ("rock", "mixed", "eight"))
def test_certified_edges(fresh_world, torch_cuda, kind):
    torch = torch_cuda
    from ca_ref import reduce_items
    from cloud_continuous_ref import EXIT_CAP
    x = _x("c2", kind)
    s, g = hk.ca_edges(x)
    g[7] = s[7]                                                  # a degenerate edge
    for scan in hcc.SCANS:
        cloud, pts, r = _cloud(scan)
        for mode, maxd, thr, la in (("connect", MAXD, 0.0, np.inf), ("connect", MAXD, 0.01, 0.05), ("steer", 0.12, 0.0, 0.05)):
            ref = hk.edge_ca_ref(x, pts, r, s, g, maxd, mode, thr, la)
            what = f"{kind} {scan} {mode} thr={thr} look_ahead={la}"
            assert (ref[3] == FREE).sum() >= 5 and (ref[3] == COLLISION).sum() >= 5, what
            assert (ref[6][EXIT_CAP] > 0) == (la == 0.05), f"{what}: items stop inside the cap with look_ahead = 0.05 only"
            for E in hk.EDGE_COUNTS:
                got = x.dev.held_cloud_edge_continuous(x.held, cloud, s[:E], g[:E], maxd, mode=mode, threshold=thr, look_ahead=la)
                assert got[0].dtype == bool
                _same_ca(got, tuple(a[:E] for a in ref[:4]), f"{what} E={E}")
                assert_bitwise(_np(got[1]), ref[1][:E], f"{what} E={E}: end")
        # accumulated into the scene's certified result, with one grasp tensor
        G = x.spec.G @ hc.rot_pose(np.random.default_rng(4), 0.4, 0.03) @ hc.trans(0, 0, -hc.BOX_Z)
        own = hk.edge_ca_ref(x, pts, r, s, g, look_ahead=0.05, G=G)
        a, Tf, live = _scene_items(x, s, g, MAXD, "connect", 0.0)
        both = reduce_items(np.concatenate((a[4], own[4]), axis=1), np.concatenate((a[5], own[5]), axis=1), Tf, live)
        assert (both[2] != a[3]).sum() >= 2, "the held object against the scan changes edges the scene decides otherwise"
        st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
        res = x.dev.edge_continuous(st, gt, MAXD, max_iter=hk.MAX_ITER)
        out = (res[0], res[2], res[3])
        got = x.dev.held_cloud_edge_continuous(x.held, cloud, st, gt, MAXD, look_ahead=0.05, pose=torch.from_numpy(G).cuda(), out=out)
        assert got[0] is res[0] and got[2] is res[2] and got[3] is res[3]
        _same_ca(out, both, f"{kind} {scan}: accumulated, a grasp tensor")
        bad = G.copy(); bad[1, 1] = np.inf
        v, e, t, stt = x.dev.held_cloud_edge_continuous(x.held, cloud, s, g, MAXD, pose=bad)
        live7 = np.arange(len(v)) != 7
        assert not v.any() and np.isnan(t[live7]).all(), "a grasp that is not finite: 0 / NaN / UNDECIDED"


@pytest.mark.parametrize("degree", (1, 3))
def test_certified_splines(fresh_world, torch_cuda, degree):
    torch = torch_cuda
    from ca_ref import reduce_items
    from spline_continuous_ref import reference_spline_continuous, degenerate
    for kind in ("mixed", "eight"):
        x = _x("c2", kind)
        ctrl, knots = hk.ca_splines(x, degree)
        for scan in hcc.SCANS:
            cloud, pts, r = _cloud(scan)
            for thr, la in ((0.0, np.inf), (0.01, 0.05)):
                ref = hk.spline_ca_ref(x, pts, r, ctrl, knots, degree, thr, la)
                what = f"{kind} degree {degree} {scan} thr={thr} look_ahead={la}"
                assert (ref[2] == FREE).sum() >= 5 and (ref[2] == COLLISION).sum() >= 5, what
                for S in hk.SPLINE_COUNTS:
                    got = x.dev.held_cloud_spline_continuous(x.held, cloud, ctrl[:S], knots, degree, threshold=thr, look_ahead=la)
                    assert got[0].dtype == bool
                    _same_ca(got, tuple(a[:S] for a in ref[:3]), f"{what} S={S}")
        # accumulated into the scene's certified result, with one grasp tensor
        G = x.spec.G @ hc.rot_pose(np.random.default_rng(4), 0.4, 0.03) @ hc.trans(0, 0, -hc.BOX_Z)
        own = hk.spline_ca_ref(x, pts, r, ctrl, knots, degree, 0.0, 0.05, G=G)
        a = reference_spline_continuous(x.sm, Oracle(x.sm), ctrl, knots, degree, threshold=0.0, max_iter=hk.MAX_ITER, slack=1e-6)
        live = ~degenerate(ctrl, np.asarray(knots, dtype=np.float64), degree)
        both = reduce_items(np.concatenate((a[3], own[3]), axis=1), np.concatenate((a[4], own[4]), axis=1), np.ones(len(live)), live)
        ct = torch.from_numpy(ctrl).cuda()
        out = x.dev.spline_continuous(ct, knots, degree, max_iter=hk.MAX_ITER)
        got = x.dev.held_cloud_spline_continuous(x.held, cloud, ct, knots, degree, look_ahead=0.05, pose=torch.from_numpy(G).cuda(), out=out)
        assert all(p is q_ for p, q_ in zip(got, out))
        _same_ca(got, both, f"{kind} degree {degree}: accumulated, a grasp tensor")


# ---- 6. the same call again gives the same bits ----------------------------------------------------------------------------------------
def test_repeats_are_bit_equal(fresh_world, torch_cuda):
    """The H = 8 attachment of hulls and primitives: the verdict call on rows, then on edges, then on splines, five times each on the
    same inputs -- every call bit-equal to the first and to the oracle (a spilled build of the primitive verdict kernels once lost
    hits from one call to the next on H = 8 rows and then edges: DESIGN.md 3)."""
    torch = torch_cuda
    x = _x("c2", "eight")
    cloud, pts, r = _cloud("dense")
    q = x.q[:hk.N_ROWS]
    s, g = hk.edges(x)
    ctrl, knots = hk.splines(x, 3)
    ref_rows = hk.mask(x.sm, x.spec, pts, r, q, 0.0)
    ref_edges = hk.edges_ref(x.sm, x.spec, pts, r, s, g)
    ref_splines = hk.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, 3)
    _mixed(ref_rows, "rows"); _mixed(ref_edges[0], "edges"); _mixed(ref_splines[0], "splines")
    qt, st, gt, ct = (torch.from_numpy(a).cuda() for a in (q, s, g, ctrl))
    for k in range(5):
        got = _np(x.dev.held_cloud_validity(x.held, cloud, qt, 0.0))
        assert np.array_equal(got.astype(bool), ref_rows), f"rows, call {k}: differs at {np.flatnonzero(got.astype(bool) != ref_rows)[:8]}"
        words = _np(x.dev.held_cloud_validity(x.held, cloud, qt, 0.0, packed=True))
        assert np.array_equal(words, hc.pack_bits(ref_rows)), f"rows, packed, call {k}"
    for k in range(5):
        _same3(x.dev.held_cloud_edge_validity(x.held, cloud, st, gt, RES, MAXD), ref_edges, f"edges, call {k}")
    for k in range(5):
        _same3(x.dev.held_cloud_spline_validity(x.held, cloud, ct, knots, 3, RES), ref_splines, f"splines, call {k}")


# ---- 7. cloud states -------------------------------------------------------------------------------------------------------------------
def test_cloud_states(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    x = _x("c2", "mixed")
    q = x.q[:130]
    s, g = hk.ca_edges(x, 65)
    ctrl, knots = hk.ca_splines(x, 3, S=33)
    pts, r = hcc.scan("dense")
    n_s = hk.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, 3)[2]
    # an empty cloud: all free, clearance inf, certified FREE at the stop point
    empty = PointCloud(np.zeros((0, 3)), 0.01, bounds=([-1, -1, 0], [1, 1, 1]), capacity=8)
    assert not x.dev.held_cloud_validity(x.held, empty, q, 0.0).any()
    d, sh, p = x.dev.held_cloud_clearance(x.held, empty, q, hk.D_MAX)
    assert np.isposinf(d).all() and (sh == -1).all() and (p == -1).all()
    rec = x.dev.held_cloud_records(x.held, empty, q, hk.D_MAX)
    assert np.isposinf(rec[0]).all() and (rec[1] == -1).all() and np.isnan(rec[3]).all() and (rec[4] == 0.0).all()
    assert x.dev.held_cloud_edge_validity(x.held, empty, s, g, RES, MAXD)[0].all()
    v, th, ns = x.dev.held_cloud_spline_validity(x.held, empty, ctrl, knots, 3, RES)
    assert v.all() and np.isnan(th).all() and np.array_equal(ns, n_s)
    v, e, t, st = x.dev.held_cloud_edge_continuous(x.held, empty, s, g, MAXD)
    assert v.all() and (t == 1.0).all() and (st == FREE).all()
    v, t, st = x.dev.held_cloud_spline_continuous(x.held, empty, ctrl, knots, 3)
    assert v.all() and (t == 1.0).all() and (st == FREE).all()
    # the status set by a non-finite point: every row hits, distances NaN, certified 0 / NaN / UNDECIDED; a clean update restores
    cloud = PointCloud(pts, r)
    ref = hk.mask(x.sm, x.spec, pts, r, q, 0.0)
    _mixed(ref, "rows")
    bad = pts.copy()
    bad[123, 1] = np.nan
    cloud.update(bad)
    assert cloud.status() == 2
    assert x.dev.held_cloud_validity(x.held, cloud, q, 0.0).all()
    d, sh, p = x.dev.held_cloud_clearance(x.held, cloud, q, hk.D_MAX)
    assert np.isnan(d).all() and (sh == -1).all() and (p == -1).all()
    rec = x.dev.held_cloud_records(x.held, cloud, q, hk.D_MAX, per_shape=True)
    assert np.isnan(rec[0]).all() and (rec[1] == -1).all() and np.isnan(rec[3]).all() and np.isnan(rec[4]).all()
    assert not x.dev.held_cloud_edge_validity(x.held, cloud, s, g, RES, MAXD)[0].any()
    _same3(x.dev.held_cloud_spline_validity(x.held, cloud, ctrl, knots, 3, RES),
           hk.splines_ref(x.sm, x.spec, pts, r, ctrl, knots, 3, status=2), "status set: splines")
    v, e, t, st = x.dev.held_cloud_edge_continuous(x.held, cloud, s, g, MAXD)
    assert not v.any() and np.isnan(t).all()
    v, t, st = x.dev.held_cloud_spline_continuous(x.held, cloud, ctrl, knots, 3)
    assert not v.any() and np.isnan(t).all()
    cloud.update(pts)
    assert cloud.status() == 0
    assert np.array_equal(x.dev.held_cloud_validity(x.held, cloud, q, 0.0), ref)


# ---- 8. capture ----------------------------------------------------------------------------------------------------------------------
def test_capture(fresh_world, torch_cuda):
    """One captured graph holding a verdict call and a clearance call; re-grasped by rewriting the grasp tensor, replayed once."""
    torch = torch_cuda
    x = _x("c2", "mixed")
    cloud, pts, r = _cloud("dense")
    B = 256
    q = x.q[:B]
    rng = np.random.default_rng(9)
    Gs = [x.spec.G @ hc.rot_pose(rng, 0.4, 0.03) @ hc.trans(0, 0, -hc.BOX_Z) for _ in range(2)]
    qt = torch.from_numpy(q.copy()).cuda()
    Gt = torch.from_numpy(Gs[0].copy()).cuda()

    def both():
        return x.dev.held_cloud_validity(x.held, cloud, qt, 0.0, pose=Gt), x.dev.held_cloud_clearance(x.held, cloud, qt, hk.D_MAX, pose=Gt)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                                   # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mask, (d, sh, p) = both()
    torch.cuda.current_stream().wait_stream(side)
    Gt.copy_(torch.from_numpy(Gs[1].copy()).cuda())
    graph.replay()
    torch.cuda.synchronize()
    ref = hk.mask(x.sm, x.spec, pts, r, q, 0.0, Gs[1])
    _mixed(ref, "the replay's grasp")
    assert (ref != hk.mask(x.sm, x.spec, pts, r, q, 0.0, Gs[0])).any(), "the two grasps give different verdicts"
    assert np.array_equal(_np(mask).astype(bool), ref), "replay: verdicts"
    dr, sr, pr = hk.closest(x.sm, x.spec, pts, r, q, hk.D_MAX, Gs[1])
    assert_bitwise(_np(d), dr, "replay: clearance")
    assert np.array_equal(_np(sh), sr) and np.array_equal(_np(p), pr)


# ---- 9. the public layer -----------------------------------------------------------------------------------------------------------------
def test_arm_entries(fresh_world, torch_cuda):
    torch = torch_cuda
    x = _x("c2", "rock")
    assert x.att is not None and x.att.mesh_scans and x.held.sees_scans and x.held.has_hull
    cloud, pts, r = _cloud("dense")
    q = x.q[:256]
    for thr in (0.0, hk.DEEP):
        alone, scan = hh.held_mask(x.sm, x.spec, q, thr), hk.mask(x.sm, x.spec, pts, r, q, thr)
        assert (scan & ~alone).sum() >= 5
        assert np.array_equal(x.arm.in_collision_with_attached(q, x.att, thr), alone), "cloud=None keeps today's result"
        assert np.array_equal(x.arm.in_collision_with_attached(q, x.att, thr, cloud=cloud), alone | scan)
    both = alone | scan
    for b in np.concatenate((np.flatnonzero(scan & ~alone)[:2], np.flatnonzero(~both)[:2])):
        assert x.arm.in_collision_with_attached(q[b], x.att, hk.DEEP, cloud=cloud) is bool(both[b])
    got = x.arm.in_collision_with_attached(torch.from_numpy(q).cuda(), x.att, hk.DEEP, cloud=cloud)
    assert got.is_cuda and np.array_equal(_np(got), both)
    dr, sr, pr = hk.closest(x.sm, x.spec, pts, r, q, hk.D_MAX)
    d, s, p = x.arm.attached_cloud_clearance(q, x.att, cloud, hk.D_MAX)
    assert_bitwise(d, dr, "attached_cloud_clearance")
    assert np.array_equal(s, sr) and np.array_equal(p, pr)
    raw = hk.records_raw(x, pts, r, q[:65])
    for per_shape in (False, True):
        got = x.arm.attached_cloud_proximity_jacobians(q[:65], x.att, cloud, hk.D_MAX, per_shape=per_shape)
        hr.assert_cloud_records(got, hk.records_ref(x, raw, hk.D_MAX, per_shape), f"attached_cloud_proximity_jacobians per_shape={per_shape}")
    ref = hk.records_ref(x, raw, hk.D_MAX, False)
    near, far = int(np.flatnonzero(ref[1] >= 0)[0]), int(np.flatnonzero(ref[1] < 0)[0])
    prox = x.arm.attached_cloud_closest_to(q[near], x.att, cloud, hk.D_MAX)
    assert prox is not None and prox.subject is x.att.objects[0] and prox.target is cloud
    assert_bitwise(np.array([prox.distance]), ref[0][near:near + 1], "attached_cloud_closest_to: distance")
    assert_bitwise(prox.position_on_subject, ref[3][near, 0:3], "attached_cloud_closest_to: the point on the rock")
    assert x.arm.attached_cloud_closest_to(q[far], x.att, cloud, hk.D_MAX) is None


def test_discrete_connector(fresh_world, torch_cuda):
    from numbotics_amd.physics import PointCloud
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, DiscreteConnector
    import cloud_cases as cc
    x = _x("c2", "rock")
    pts, r = hcc.scan("sparse")
    cloud = PointCloud(pts, r)
    s, g = hk.edges(x)
    kw = dict(arm=x.arm, cloud=cloud, cloud_ignore_links=(x.base,), attached=x.att, resolution=RES, max_distance=hcc.MAXD_STEER)
    con = DiscreteConnector(ConnectorParams(attached_sees_cloud=True, **kw))
    blind = DiscreteConnector(ConnectorParams(**kw))
    both_m = hh.held_model_hulls(x.sm, x.spec, keep_scene=True)
    for m in ("connect", "steer"):
        a = Oracle(both_m).edge_validity(s, g, RES, hcc.MAXD_STEER, mode=m, nthreads=8)
        b = hcc.arm_cloud_edges_ref(x.sm, pts, r, s, g, hcc.MAXD_STEER, m, shapes=x.shapes)
        c = hk.edges_ref(x.sm, x.spec, pts, r, s, g, hcc.MAXD_STEER, m)
        three, four = a[0] & b[0], a[0] & b[0] & c[0]
        _mixed(four, f"connector {m}")
        assert (three & ~four).sum() >= 3, "the flag must reject edges the three steps accept"
        if m == "connect":
            assert np.array_equal(con.connect_batch(s, g), four)
            assert np.array_equal(blind.connect_batch(s, g), three)
        else:
            ok, end = con.steer_batch(s, g)
            assert np.array_equal(ok, four)
            assert_bitwise(end, a[1], "steer end states")
    q = x.q[:32]
    hit3 = Oracle(both_m).validity(q, 0.0) | cc.cloud_mask(x.sm, pts, r, q, 0.0, shapes=x.shapes)
    hit4 = hit3 | hk.mask(x.sm, x.spec, pts, r, q, 0.0)
    assert np.array_equal(np.array([con.is_valid(q[b]) for b in range(32)]), ~hit4)
    assert np.array_equal(np.array([blind.is_valid(q[b]) for b in range(32)]), ~hit3)


def test_the_rock_carried_through_a_scanned_wall(fresh_world, torch_cuda):
    """The edge of tests/test_held_hull_cloud_host.py: accepted by the certificate that does not look at the held rock against the
    scan, rejected by the one that does."""
    from numbotics_amd.physics import PointCloud
    from numbotics_amd.planning.sampling_based.connectors import ConnectorParams, ContinuousConnector
    x = _x("c2", "rock")
    out = hk.wall_edge(x)
    assert out is not None
    pts, r, s, g, t_held, cross = out
    wall = PointCloud(pts, r)
    kw = dict(cloud=wall, cloud_ignore_links=(x.base,), attached=x.att, max_iter=hk.MAX_ITER)
    p = ConnectorParams(arm=x.arm, max_distance=MAXD)
    blind = ContinuousConnector(p, **kw)
    seeing = ContinuousConnector(p, attached_sees_cloud=True, **kw)
    valid, end, t_free, status = blind.certify_batch(s[None], g[None])
    assert valid[0] and status[0] == FREE and t_free[0] == 1.0, "without the flag the edge through the wall is called FREE"
    assert blind.connect(s, g) is not None
    valid, end, t_free, status = seeing.certify_batch(s[None], g[None])
    assert not valid[0] and status[0] == COLLISION and t_free[0] == t_held < cross
    assert seeing.connect(s, g) is None and seeing.steer(s, g) is None


# ---- 10. what is still refused ---------------------------------------------------------------------------------------------------------
def test_refusals_that_remain(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd import _lib
    from numbotics_amd.physics import Plane, PointCloud
    x = _x("c2", "rock", scans=False)
    assert x.held.has_hull and not x.held.sees_scans and not x.att.mesh_scans
    q = x.q[:65]
    s, g = hk.ca_edges(x, 65)
    ctrl, knots = hk.ca_splines(x, 3, S=8)
    cloud, pts, r = _cloud("sparse")
    calls = lambda held, att: (                                                                           # noqa: E731
        lambda: x.dev.held_cloud_validity(held, cloud, q), lambda: x.dev.held_cloud_clearance(held, cloud, q, 0.1),
        lambda: x.dev.held_cloud_records(held, cloud, q, 0.1), lambda: x.dev.held_cloud_edge_validity(held, cloud, s, g, RES, MAXD),
        lambda: x.dev.held_cloud_spline_validity(held, cloud, ctrl, knots, 3, RES),
        lambda: x.dev.held_cloud_edge_continuous(held, cloud, s, g, MAXD),
        lambda: x.dev.held_cloud_spline_continuous(held, cloud, ctrl, knots, 3),
        lambda: x.arm.in_collision_with_attached(q, att, cloud=cloud), lambda: x.arm.attached_cloud_clearance(q, att, cloud, 0.1),
        lambda: x.arm.attached_cloud_proximity_jacobians(q, att, cloud, 0.1), lambda: x.arm.attached_cloud_closest_to(q[0], att, cloud, 0.1))
    for f in calls(x.held, x.att):
        with pytest.raises(ValueError, match=MSG):
            f()
    # at the C boundary: an unflagged object is NBK_ERR_UNSUPPORTED and nothing is written; the flag set, the same call is served;
    # cleared again, it is refused again
    lib = _lib.load()
    qt = torch.from_numpy(q).cuda()
    m = torch.full((65,), 7, dtype=torch.uint8, device="cuda")
    d = torch.full((65,), 7.0, dtype=torch.float64, device="cuda")
    M, H, Cl = x.dev._h, x.held._h, cloud._h
    assert lib.nbk_held_cloud_validity_batch(M, H, Cl, qt.data_ptr(), 65, None, 0, 0.0, 0, None, m.data_ptr(), None) == -4
    assert lib.nbk_held_cloud_clearance_batch(M, H, Cl, qt.data_ptr(), 65, None, 0, 0.1, d.data_ptr(), None, None, None) == -4
    torch.cuda.synchronize()
    assert (m == 7).all() and (d == 7.0).all(), "a refused call writes nothing"
    assert lib.nbk_held_set_cloud_hulls(H, 1) == 0
    assert lib.nbk_held_cloud_validity_batch(M, H, Cl, qt.data_ptr(), 65, None, 0, 0.0, 0, None, m.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy().astype(bool), hk.mask(x.sm, x.spec, pts, r, q, 0.0))
    assert lib.nbk_held_set_cloud_hulls(H, 0) == 0
    assert lib.nbk_held_cloud_validity_batch(M, H, Cl, qt.data_ptr(), 65, None, 0, 0.0, 0, None, m.data_ptr(), None) == -4
    # a flagged attachment is refused by nothing; an object without hulls takes the flag and is served as before
    seen = x.arm.attach(x.att.objects[0], "gripper", pose=hh.GRASP["rock"], meshes=True, mesh_scans=True)
    dev, held = seen._device(x.arm)
    assert dev is x.dev
    for f in calls(held, seen):
        f()
    box_att, box = hc.gripper_box(x.arm)
    bspec = box_att.spec(x.arm)
    prim = hk.device_held(x.dev, bspec, scans=True)
    plain = hk.device_held(x.dev, bspec, scans=False)
    assert not prim.has_hull and prim.sees_scans
    ref = hcc.mask(x.sm, bspec, pts, r, q, 0.0)
    assert np.array_equal(x.dev.held_cloud_validity(prim, cloud, q), ref) and np.array_equal(x.dev.held_cloud_validity(plain, cloud, q), ref)
    # a PLANE is refused either way
    pl = Plane(0.0, np.array([0.0, 0.0, 1.0]), position=hc.PARK.copy())
    for kw in (dict(), dict(meshes=True), dict(meshes=True, mesh_scans=True)):
        with pytest.raises(ValueError, match="PLANE"):
            x.arm.attach(pl, "gripper", pose=np.eye(4), **kw)
