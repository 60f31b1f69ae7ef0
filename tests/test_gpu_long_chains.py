"""Every entry point on the size ladder of 9- to 32-joint robots (tests/long_chain_cases.py), bit for bit against the CPU oracle:
k_fk<false> at n_q 9 .. 32, k_jacobian on paths of 9 .. 32 joints, k_jacobian_reg<8> on short paths inside long robots and
against k_jacobian on the same input, k_ik up to its LDS limit and its refusal beyond, validity / edges / trajectories / item
records on robots up to and beyond the LDS-parked layout, and the all-pairs entry points just under and just over their limits:
an entry point whose restated LDS need (long_chain_cases.lds_need) is within the limit must serve the robot, one beyond it either
serves it correctly or says NBK_ERR_UNSUPPORTED.  test_long_chains_host.py checks the inputs and pins the oracle on these robots.
Needs a real MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd._lib import NbkError, debug_option
from test_gpu_parity import assert_bitwise, fused_path, torch_cuda      # noqa: F401  (fixture)
import long_chain_cases as L
from long_chain_cases import BATCHES, LDS_MAX

B_MAX = max(BATCHES)


def _served(fn, must_serve, what):
    """fn() -> its result, or None after a refusal: NbkError with NBK_ERR_UNSUPPORTED, allowed only when ``must_serve`` is False."""
    try:
        return fn()
    except NbkError as e:
        assert "NBK_ERR_UNSUPPORTED" in str(e), f"{what}: {e}"
        assert not must_serve, f"{what}: refused although the restated LDS need is within the limit ({e})"
        return None


def _poses(n, seed):
    """n proper rigid poses (4x4)."""
    from geom_truth import random_pose
    rng = np.random.default_rng(seed)
    return np.array([random_pose(rng, 0.3) for _ in range(n)])


def _off_by_8(torch, a):
    """A device view of ``a`` that starts 8 bytes past a 16-byte boundary."""
    slab = torch.from_numpy(np.concatenate(([0.0], np.ascontiguousarray(a, dtype=np.float64).ravel()))).cuda()
    view = slab[1:]
    assert view.data_ptr() % 16 == 8
    return view


# ---- kinematics -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.NAMES)
def test_fk(name, tmp_path, torch_cuda):
    arm, chain, obs = L.case(name, tmp_path)
    kin = arm._kin
    assert kin.n_q > 8                                   # k_fk<false>
    orc, dev = Oracle(kin), arm._kin_device()
    q = L.sample(chain, B_MAX, 113)
    deep = L.deepest_frame(kin)
    frames = list(dict.fromkeys(L.probe_frames(kin) + [deep]))
    ref = {f: orc.fk(q, f) for f in frames}
    for B in BATCHES:
        for f in frames:
            assert_bitwise(dev.fk(q[:B], f), ref[f][:B], f"{name} fk {f} B={B}")
    for B in (B_MAX, 65):
        view = _off_by_8(torch_cuda, q[:B])
        assert_bitwise(dev.fk(view, deep).cpu().numpy(), ref[deep][:B], f"{name} fk from a misaligned q, B={B}")
    lp = _poses(B_MAX, 5)
    assert_bitwise(dev.fk(q, deep, local_pose=lp), orc.fk(q, deep, local_pose=lp), f"{name} fk local_pose")
    # every link frame in one sweep
    names = list(kin.link_names)
    must = L.served(None, kin, "fk_frames")
    for B in (B_MAX, 63):
        T = _served(lambda: dev.fk_frames(q[:B], names), must, f"{name} fk_frames")
        if T is not None:
            for i, f in enumerate(names):
                want = ref[f][:B] if f in ref else orc.fk(q[:B], f)
                assert_bitwise(T[:, i], want, f"{name} fk_frames {f} B={B}")


@pytest.mark.parametrize("name", L.NAMES)
def test_jacobian(name, tmp_path, torch_cuda):
    torch = torch_cuda
    arm, chain, obs = L.case(name, tmp_path)
    kin = arm._kin
    orc, dev = Oracle(kin), arm._kin_device()
    q = L.sample(chain, B_MAX, 113)
    paths = L.frames_by_path(kin)
    deep = L.deepest_frame(kin)
    assert len(kin.frames[deep].path) > 8 and L.served(None, kin, "jacobian")
    frames = [deep, paths[8], paths[9], paths[3]]
    short = [paths[8], paths[3]]                          # k_jacobian_reg<8> inside a robot with n_q > 8
    gp, lp = _poses(B_MAX, 7), _poses(B_MAX, 9)
    ref = {}
    for f in frames:
        ref[f, "plain"] = orc.jacobian(q, f)
        ref[f, "global"] = orc.jacobian(q, f, global_pose=gp)
        ref[f, "one global"] = orc.jacobian(q, f, global_pose=np.tile(gp[:1], (B_MAX, 1, 1)))
        ref[f, "local"] = orc.jacobian(q, f, local_pose=lp)

    def run(f, B, mode):
        if mode == "plain":
            return arm.jacobian(q[:B], f)
        if mode == "global":
            return arm.jacobian(q[:B], f, global_pose=gp[:B])
        if mode == "one global":
            return arm.jacobian(q[:B], f, global_pose=gp[0])
        return arm.jacobian(q[:B], f, local_pose=lp[:B])

    for B in BATCHES:
        for f in frames:
            for mode in ("plain", "global", "one global", "local"):
                got = run(f, B, mode)
                assert_bitwise(got, ref[f, mode][:B], f"{name} jacobian {f} ({len(kin.frames[f].path)} joints) {mode} B={B}")
                if f in short:
                    with debug_option("jac_two_sweep", 1):
                        two = run(f, B, mode)
                    assert_bitwise(two, got, f"{name} k_jacobian vs k_jacobian_reg {f} {mode} B={B}")
    # an output slab that is only 8-byte aligned, through the C-ABI
    for f in (deep, paths[3]):
        for B in (B_MAX, 63):
            path, local = dev._frame_args(f, None)
            qt = torch.from_numpy(q[:B]).cuda()
            slab = torch.full((B * 6 * kin.n_q + 1,), -7.0, dtype=torch.float64, device="cuda")
            out = slab[1:]
            assert out.data_ptr() % 16 == 8
            assert dev._lib.nbk_jacobian_batch(dev._h, qt.data_ptr(), B, path.ctypes.data, len(path), local.ctypes.data, 0, None,
                                               out.data_ptr(), dev._stream()) == 0
            torch.cuda.synchronize()
            assert_bitwise(out.cpu().numpy().reshape(B, 6, kin.n_q), ref[f, "plain"][:B], f"{name} jacobian {f} into a misaligned slab B={B}")
            assert float(slab[0]) == -7.0


def _check_ik(dev, orc, chain, kin, frame, n, limits, what):
    pose, q0 = L.ik_problems(orc, chain, frame, n)
    okr, qr, nrmr, itr = orc.ik(pose, q0, frame, limits=limits)
    ok, q, nrm, it = dev.ik(pose, q0, frame, limits=limits)
    assert np.array_equal(ok, okr), f"{what}: success flags differ on {np.flatnonzero(ok != okr)[:10]}"
    assert np.array_equal(it, itr), f"{what}: step counts differ on {np.flatnonzero(it != itr)[:10]}"
    assert_bitwise(q, qr, f"{what} q")
    assert_bitwise(nrm, nrmr, f"{what} residual")
    on_path = {int(kin.joint_qidx[k]) for k in kin.frames[frame].path}
    off = [c for c in range(kin.n_q) if c not in on_path]
    if limits is None:
        assert np.array_equal(q[:, off], q0[:, off]), f"{what}: joints off the path moved"
    else:               # a step clips the whole row to the limits; nothing else touches a joint off the path
        clipped = np.clip(q0, limits[:, 0], limits[:, 1])
        assert ((q[:, off] == q0[:, off]) | (q[:, off] == clipped[:, off])).all(), f"{what}: joints off the path moved"
    return ok


@pytest.mark.parametrize("name,path_len", L.IK_CASES, ids=[c for c, _ in L.IK_CASES])
def test_ik_up_to_the_lds_limit(name, path_len, tmp_path, torch_cuda):
    """k24's full path is the last one served: 512 (7 * 24 + 6 * 24) = 159 744 of 163 840 bytes."""
    arm, chain, obs = L.case(name, tmp_path)
    kin = arm._kin
    orc, dev = Oracle(kin), arm._kin_device()
    frame = L.ik_frame(kin, path_len)
    n_path = len(kin.frames[frame].path)
    assert L.lds_need(None, kin, "ik", n_path) <= LDS_MAX
    if name == "k24":
        assert n_path == 24 and L.lds_need(None, kin, "ik", n_path) == 159744
    lim = np.asarray(chain.joint_limits, dtype=np.float64)
    for limits in (None, lim):
        ok = _check_ik(dev, orc, chain, kin, frame, 1000, limits, f"{name} ik {frame} limits={limits is not None}")
        assert ok.mean() >= 0.9
    for B in (1, 63, 65):
        _check_ik(dev, orc, chain, kin, frame, B, None, f"{name} ik {frame} B={B}")


def test_ik_leaves_joints_off_the_path_alone(tmp_path, torch_cuda):
    arm, chain, obs = L.case("tree", tmp_path)
    kin = arm._kin
    orc, dev = Oracle(kin), arm._kin_device()
    paths = L.frames_by_path(kin)
    deep = L.deepest_frame(kin)
    for frame in (deep, paths[8], paths[3]):
        assert len(kin.frames[frame].path) < kin.n_q
        _check_ik(dev, orc, chain, kin, frame, 500, None, f"tree ik {frame}")


@pytest.mark.parametrize("name", ["k25", "k32s", "k32d"])
def test_ik_refusal(name, tmp_path, torch_cuda):
    """The full path needs more than 160 KB: the call is refused before the launch (or, should the library learn to serve it,
    served correctly); a served call after the refusal is still right, and every path whose need is within the limit is served."""
    arm, chain, obs = L.case(name, tmp_path)
    kin = arm._kin
    orc, dev = Oracle(kin), arm._kin_device()
    deep = L.deepest_frame(kin)
    assert L.lds_need(None, kin, "ik", len(kin.frames[deep].path)) > LDS_MAX
    paths = L.frames_by_path(kin)
    longest = max(n for n in paths if L.lds_need(None, kin, "ik", n) <= LDS_MAX)
    assert L.lds_need(None, kin, "ik", longest + 1) > LDS_MAX and longest >= 12
    for frame, must in ((deep, False), (paths[longest], True), (paths[longest + 1], False), (paths[9], True)):
        got = _served(lambda: _check_ik(dev, orc, chain, kin, frame, 200, None, f"{name} ik {frame}"), must, f"{name} ik {frame}")
    q = L.sample(chain, 65, 113)
    assert_bitwise(dev.fk(q, deep), orc.fk(q, deep), f"{name} fk after a refusal")


# ---- collision --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.NAMES)
def test_validity(name, tmp_path, torch_cuda):
    arm, chain, obs = L.case(name, tmp_path)
    sm, dev = arm._scene_device()
    orc = Oracle(sm)
    q = L.collision_q(name, chain)
    for thr in L.THRESHOLDS:
        ref = orc.validity(q, thr, nthreads=8)
        got = dev.validity(q, thr)
        used = dev.broad_kernel_used()
        assert np.array_equal(got, ref), f"{name} thr={thr}: {(got != ref).sum()} verdicts differ (broadphase {used})"
        with fused_path():
            got = np.concatenate([dev.validity(q[i:i + 1400], thr) for i in range(0, len(q), 1400)])
        assert np.array_equal(got, ref), f"{name} thr={thr} fused: {(got != ref).sum()} verdicts differ"
        for option in ("no_reg_broad", "f64_broad"):
            with debug_option(option, 1):
                got = dev.validity(q, thr)
                used = dev.broad_kernel_used()
            assert np.array_equal(got, ref), f"{name} thr={thr} {option}: {(got != ref).sum()} verdicts differ (broadphase {used})"
        assert np.array_equal(dev.validity(q[:100], thr), ref[:100]), f"{name} thr={thr} batch of 100"
        assert dev.validity_scalar(q[7], thr) == bool(ref[7]) and dev.validity_scalar(q[8], thr) == bool(ref[8])


@pytest.mark.parametrize("name", L.NAMES)
def test_edges(name, tmp_path, torch_cuda):
    from continuous_ref import reference_continuous, DEGENERATE
    arm, chain, obs = L.case(name, tmp_path)
    sm, dev = arm._scene_device()
    orc = Oracle(sm)
    s, g = L.edges(name, chain)
    for mode in ("connect", "steer"):
        for thr in (0.0, 0.01):
            ok, end, ns = dev.edge_validity(s, g, L.EDGE_RESOLUTION, L.MAX_DISTANCE[mode], mode=mode, threshold=thr)
            okr, endr, nsr = orc.edge_validity(s, g, L.EDGE_RESOLUTION, L.MAX_DISTANCE[mode], mode=mode, threshold=thr, nthreads=8)
            assert np.array_equal(ok, okr), f"{name} {mode} thr={thr}: verdicts differ on {np.flatnonzero(ok != okr)[:10]}"
            assert np.array_equal(ns, nsr), f"{name} {mode} thr={thr}: sample counts differ"
            assert_bitwise(end, endr, f"{name} {mode} thr={thr} end states")
            if thr == 0.0:
                # the one-wave-per-edge kernel parks the whole robot (tree: 1 792 B under the limit); robots beyond the layout ignore the switch
                with debug_option("edge_batch_min_e", 10 ** 9):
                    ok1, end1, ns1 = dev.edge_validity(s, g, L.EDGE_RESOLUTION, L.MAX_DISTANCE[mode], mode=mode)
                assert np.array_equal(ok1, okr) and np.array_equal(ns1, nsr), f"{name} {mode}: one wave per edge differs"
                assert_bitwise(end1, endr, f"{name} {mode} end states, one wave per edge")
                one = dev.edge_validity_scalar(s[3], g[3], L.EDGE_RESOLUTION, L.MAX_DISTANCE[mode], mode=mode)
                assert one[0] == bool(okr[3]) and one[2] == nsr[3], f"{name} {mode}: scalar edge call differs"
                assert_bitwise(one[1], endr[3], f"{name} {mode} scalar edge end state")
    # certified: a handful against the restatement of the loop, all of them against a fine sampled check
    n = L.N_CERTIFIED
    for mode, thr, m in (("connect", 0.0, n), ("steer", 0.01, L.N_CERTIFIED_STEER)):
        got = dev.edge_continuous(s[:m], g[:m], L.MAX_DISTANCE[mode], mode=mode, threshold=thr)
        rv, rend, rtf, rst = reference_continuous(sm, orc, s[:m], g[:m], L.MAX_DISTANCE[mode], mode=mode, threshold=thr)[:4]
        assert np.array_equal(got[0], rv) and np.array_equal(got[3], rst), f"{name} certified {mode}: verdict / status differ"
        assert_bitwise(got[2], rtf, f"{name} certified {mode} t_free")
        assert_bitwise(got[1], rend, f"{name} certified {mode} end")
    valid, _, t_free, status = dev.edge_continuous(s, g, L.MAX_DISTANCE["connect"])
    assert np.array_equal(valid[:n], dev.edge_continuous(s[:n], g[:n], L.MAX_DISTANCE["connect"])[0])
    assert (status != DEGENERATE).all()
    fine = dev.edge_validity(s, g, 0.01, L.MAX_DISTANCE["connect"])[0]
    assert not (valid & ~fine).any(), f"{name}: {int((valid & ~fine).sum())} edges certified free fail a sampled check"
    assert 0.1 <= valid.mean() <= 0.9, valid.mean()


@pytest.mark.parametrize("name", L.SPLINE_CASES)
def test_splines(name, tmp_path, torch_cuda):
    from numbotics_amd.planning import unit_knots
    from spline_ref import reference_splines
    from spline_continuous_ref import reference_spline_continuous
    arm, chain, obs = L.case(name, tmp_path)
    sm, dev = arm._scene_device()
    orc = Oracle(sm)
    n = L.N_CERTIFIED_SPLINES
    for k, n_ctrl in L.SPLINE_SHAPES:
        c = L.splines(name, chain, n_ctrl)
        kn = unit_knots(n_ctrl, k)
        for thr in (0.0, 0.01):
            v, th, ns = dev.spline_validity(c, kn, k, L.SPLINE_RESOLUTION, threshold=thr)
            rv, rth, rns = reference_splines(orc, c, kn, k, L.SPLINE_RESOLUTION, threshold=thr)
            assert np.array_equal(ns, rns) and np.array_equal(v, rv), f"{name} k={k} thr={thr}: sampled verdicts differ"
            assert_bitwise(th, rth, f"{name} k={k} thr={thr} t_hit")
        got = dev.spline_continuous(c[:n], kn, k)
        rv, rtf, rst = reference_spline_continuous(sm, orc, c[:n], kn, k)[:3]
        assert np.array_equal(got[0], rv) and np.array_equal(got[2], rst), f"{name} k={k}: certified verdict / status differ"
        assert_bitwise(got[1], rtf, f"{name} k={k} certified t_free")
        valid = dev.spline_continuous(c, kn, k)[0]
        fine = dev.spline_validity(c, kn, k, 0.01)[0]
        assert not (valid & ~fine).any(), f"{name} k={k}: trajectories certified free fail a sampled check"
        assert 0.1 <= valid.mean() <= 0.9, (k, valid.mean())


@pytest.mark.parametrize("name", L.NAMES)
def test_item_records(name, tmp_path, torch_cuda):
    """nbk_pair_records_items parks nothing, so it serves every descriptor, k32d (beyond the parked layout) included."""
    arm, chain, obs = L.case(name, tmp_path)
    sm, dev = arm._scene_device()
    orc = Oracle(sm)
    assert L.lds_need(sm, sm.kin, "records") <= LDS_MAX
    B, P = 64, sm.n_pairs
    q = L.collision_q(name, chain)[:B]
    dr, wr, rr = orc.proximity_jacobian(q)
    assert (dr < 0).any() and (dr > 0).any()
    rng = np.random.default_rng(131)
    items = np.stack((rng.integers(0, B, 2048), rng.integers(0, P, 2048)), axis=1).astype(np.int32)
    bad = np.array([[-1, 0], [B, 1], [3, -1], [3, P], [-5, P + 2], [B + 63, P - 1]], dtype=np.int32)
    where = rng.permutation(2048)[:len(bad)]
    items[where] = bad
    inside = np.ones(2048, dtype=bool)
    inside[where] = False
    for N in (2048, 65):
        it, keep = items[:N], inside[:N]
        b, p = it[keep, 0], it[keep, 1]
        d, w, j = dev.pair_records(q, it)
        assert_bitwise(d[keep], dr[b, p], f"{name} N={N} item distances")
        assert_bitwise(w[keep], wr[b, p], f"{name} N={N} item witnesses")
        assert_bitwise(j[keep], rr[b, p], f"{name} N={N} item rows")
        assert np.isnan(d[~keep]).all() and np.isnan(w[~keep]).all() and np.isnan(j[~keep]).all()
        d2, _, j2 = dev.pair_records(q, it, witness=False)
        assert_bitwise(d2, d, f"{name} N={N} distances without witnesses")
        assert_bitwise(j2, j, f"{name} N={N} rows without witnesses")


@pytest.mark.parametrize("name", L.NAMES)
def test_all_pairs_entry_points(name, tmp_path, torch_cuda):
    """closest / pair_distances / proximity_jacobian: served and bit-equal where the restated need is within the limit (tree
    256 B under the distances limit, k24 256 B under the proximity limit), served correctly or refused where it is beyond."""
    arm, chain, obs = L.case(name, tmp_path)
    sm, dev = arm._scene_device()
    kin = sm.kin
    orc = Oracle(sm)
    q = L.collision_q(name, chain)[:B_MAX]
    need = {w: L.lds_need(sm, kin, w) for w in ("parked", "distances", "proximity")}
    for B in (B_MAX, 63):
        must = L.served(sm, kin, "parked")
        got = _served(lambda: dev.closest(q[:B]), must, f"{name} closest ({need})")
        if got is not None:
            dref, iref = orc.closest(q[:B])
            assert_bitwise(got[0], dref, f"{name} closest distance B={B}")
            assert np.array_equal(got[1], iref), f"{name} closest pair B={B}"
            with debug_option("closest_brute", 1):
                d2, i2 = dev.closest(q[:B])
            assert_bitwise(d2, dref, f"{name} closest (brute) distance B={B}")
            assert np.array_equal(i2, iref)
        must = L.served(sm, kin, "distances")
        got = _served(lambda: dev.pair_distances(q[:B], witness=True), must, f"{name} pair_distances ({need})")
        if got is not None:
            dref, wref = orc.pair_distances(q[:B], witness=True)
            assert_bitwise(got[0], dref, f"{name} pair distances B={B}")
            assert_bitwise(got[1], wref, f"{name} pair witnesses B={B}")
            assert_bitwise(dev.pair_distances(q[:B]), dref, f"{name} pair distances without witnesses B={B}")
        must = L.served(sm, kin, "proximity")
        got = _served(lambda: dev.proximity_jacobian(q[:B]), must, f"{name} proximity_jacobian ({need})")
        if got is not None:
            dref, wref, rref = orc.proximity_jacobian(q[:B])
            assert_bitwise(got[0], dref, f"{name} proximity distances B={B}")
            assert_bitwise(got[1], wref, f"{name} proximity witnesses B={B}")
            assert_bitwise(got[2], rref, f"{name} proximity rows B={B}")


def test_refusals_leave_the_descriptor_usable(tmp_path, torch_cuda):
    """k32d is beyond the parked layout (173 824 B): each of the three all-pairs calls is refused with NBK_ERR_UNSUPPORTED, and
    after each refusal the same descriptor still answers validity and item records correctly, on the calling stream and on a
    second one."""
    torch = torch_cuda
    arm, chain, obs = L.case("k32d", tmp_path)
    sm, dev = arm._scene_device()
    orc = Oracle(sm)
    assert not L.served(sm, sm.kin, "parked")
    q = L.collision_q("k32d", chain)[:1000]
    ref = orc.validity(q, 0.0, nthreads=8)
    dr, wr, rr = orc.proximity_jacobian(q[:64])
    rng = np.random.default_rng(137)
    items = np.stack((rng.integers(0, 64, 500), rng.integers(0, sm.n_pairs, 500)), axis=1).astype(np.int32)
    refused = 0
    for call in (lambda: dev.closest(q[:64]), lambda: dev.pair_distances(q[:64]), lambda: dev.proximity_jacobian(q[:64])):
        refused += _served(call, False, "k32d all-pairs call") is None
        assert np.array_equal(dev.validity(q, 0.0), ref), "validity after an all-pairs call on k32d"
        d, w, j = dev.pair_records(q[:64], items)
        assert_bitwise(d, dr[items[:, 0], items[:, 1]], "item distances after an all-pairs call on k32d")
        assert_bitwise(j, rr[items[:, 0], items[:, 1]], "item rows after an all-pairs call on k32d")
    assert refused == 3
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = dev.validity(q, 0.0)
        d, w, j = dev.pair_records(q[:64], items)
    side.synchronize()
    assert np.array_equal(got, ref), "validity on a second stream"
    assert_bitwise(d, dr[items[:, 0], items[:, 1]], "item distances on a second stream")
    assert_bitwise(w, wr[items[:, 0], items[:, 1]], "item witnesses on a second stream")
