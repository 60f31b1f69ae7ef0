"""The size ladder of 9- to 32-joint robots (tests/long_chain_cases.py) on the CPU: the cases are what their table says, their
configurations / edges / trajectories are neither all free nor all colliding, and the oracle's FK, Jacobian and IK on long chains
hold against long-double restatements written from the model tables alone.  The GPU file (test_gpu_long_chains.py) compares the
kernels with this oracle bit for bit on the same inputs, so whatever the oracle got wrong here the GPU parity would inherit."""
import numpy as np
import pytest

from oracle.cpu_oracle import Oracle
import long_chain_cases as L
from long_chain_cases import LDS_MAX

# name -> dof, moving joints, links, path length of the last link frame, robot shapes, frame slots, parked layout
TABLE = {
    "k9": (9, 9, 11, 9, 12, 0, True),
    "k16": (16, 16, 19, 16, 16, 0, True),
    "k18": (18, 18, 19, 18, 17, 0, True),
    "k24": (24, 24, 28, 24, 24, 0, True),
    "k25": (25, 25, 26, 25, 20, 0, True),
    "k32s": (32, 32, 33, 32, 16, 0, True),
    "k32d": (32, 32, 33, 32, 48, 0, False),
    "tree": (21, 21, 30, None, 29, 6, True),
}
NEAR = 8 * 1024            # "just under a limit": within 8 KB of it


def _model(name, tmp_path):
    arm, chain, obs = L.case(name, tmp_path)
    return arm, chain, arm.scene_model()


@pytest.mark.parametrize("name", L.NAMES)
def test_cases_are_what_the_table_says(name, tmp_path):
    arm, chain, sm = _model(name, tmp_path)
    kin = sm.kin
    dof, joints, links, last_path, shapes, slots, parked = TABLE[name]
    assert (chain.dof, kin.n_q, kin.n_joints, len(kin.link_names)) == (dof, dof, joints, links)
    assert sm.n_rshapes == shapes and 2 <= sm.n_wshapes <= 3 and sm.n_pairs > 0
    if last_path is not None:
        assert len(kin.frames[kin.link_names[-1]].path) == last_path
        assert L.CASES[name]["joints"] == joints and L.CASES[name]["shapes"] == shapes
    assert L.frame_slots(kin) == slots
    assert (L.lds_need(sm, kin, "parked") <= LDS_MAX) == parked
    paths = L.frames_by_path(kin)
    assert all(n in paths for n in (3, 8, 9)), sorted(paths)
    assert len(kin.frames[L.deepest_frame(kin)].path) > 8
    if name == "tree":
        assert dof >= 12 and slots >= 4
        assert any(len(kin.frames[f].path) < kin.n_joints and kin.frames[f].joint >= 0 for f in kin.link_names)
    if name == "k32d":
        assert kin.n_q + L.shape_rows(sm) > 315


def test_ladder_straddles_every_lds_limit(tmp_path):
    """The restated needs in bytes, per case (deepest frame for ik):

        case   parked  distances  proximity      ik  jacobian  fk_frames
        k9      36096      37632      65280   59904     32768      13312
        k16     59648      61184     110336  106496     57856      16896
        k18     62208      63744     119040  119808     65024      18432
        k24     88320      89856     163584  159744     86528      24576
        k25     75008      76544     153344  166400     90112      25600
        k32s    66304      67840     166144  212992    115200      32768
        k32d   173824     175360     273664  212992    115200      32768
        tree   162048     163584     228096  121344     75776      58368

    against LDS_MAX = 163840: tree sits 1 792 B under the parked limit and 256 B under the distances limit, k24 256 B under the
    proximity limit and 4 096 B under the IK limit; k32d is over the first two, k32s / k32d / tree over the third, k25 / k32s /
    k32d over the fourth.  The two-sweep Jacobian and fk_frames never reach the limit with at most 32 joints."""
    need = {}
    for name in L.NAMES:
        arm, chain, sm = _model(name, tmp_path)
        kin = sm.kin
        need[name] = {w: L.lds_need(sm, kin, w, len(kin.frames[L.deepest_frame(kin)].path)) for w in L.ENTRY_POINTS}
        print(name, need[name])
    for what in ("parked", "distances", "proximity", "ik"):
        under = [n for n in L.NAMES if LDS_MAX - NEAR <= need[n][what] <= LDS_MAX]
        over = [n for n in L.NAMES if need[n][what] > LDS_MAX]
        assert under and over, (what, under, over)
    assert need["k24"]["ik"] == 159744 and need["k25"]["ik"] == 166400
    assert LDS_MAX - NEAR <= need["k24"]["proximity"] <= LDS_MAX
    arm, chain, sm = _model("k32s", tmp_path)
    assert L.lds_need(sm, sm.kin, "ik", 12) == 151552
    assert all(need[n]["jacobian"] <= LDS_MAX and need[n]["fk_frames"] <= LDS_MAX for n in L.NAMES)


@pytest.mark.parametrize("name", L.NAMES)
def test_inputs_are_neither_all_free_nor_all_colliding(name, tmp_path):
    """Conditions on the inputs of the GPU file, checked with the oracle alone.  Measured when the seeds and gaps were settled
    (colliding fraction at threshold 0 / 0.01 / -0.002; valid share of the 200 edges under the sampled check, connect / steer;
    valid of the first 32 edges under the certified check; valid of the first 16 under it in steer mode at threshold 0.01):

        k9    0.47 0.56 0.45   0.48 0.50   17   5
        k16   0.46 0.52 0.45   0.43 0.47   17   6
        k18   0.58 0.65 0.56   0.33 0.39   11   5
        k24   0.38 0.44 0.36   0.51 0.58   12   7
        k25   0.56 0.63 0.55   0.27 0.32    7   4
        k32s  0.43 0.51 0.41   0.47 0.54   12   3
        k32d  0.30 0.33 0.29   0.57 0.66   12  10
        tree  0.48 0.56 0.47   0.36 0.44   11   7

    The certified share of all 200 edges is asserted in the GPU file, on the device's verdicts (the NumPy restatement of the loop
    evaluates every pair at every stop, which is seconds for 32 edges of k32d).
    """
    from continuous_ref import reference_continuous
    arm, chain, sm = _model(name, tmp_path)
    orc = Oracle(sm)
    q = L.collision_q(name, chain)
    frac = [float(orc.validity(q, thr, nthreads=8).mean()) for thr in L.THRESHOLDS]
    print(name, "colliding", frac)
    assert 0.1 <= frac[0] <= 0.9, frac
    s, g = L.edges(name, chain)
    for mode in ("connect", "steer"):
        ok = orc.edge_validity(s, g, L.EDGE_RESOLUTION, L.MAX_DISTANCE[mode], mode=mode, nthreads=8)[0]
        print(name, mode, "sampled valid", ok.mean())
        assert 0.1 <= ok.mean() <= 0.9, (mode, ok.mean())
    n = L.N_CERTIFIED
    ok = reference_continuous(sm, orc, s[:n], g[:n], L.MAX_DISTANCE["connect"])[0]
    print(name, "certified valid", int(ok.sum()), "of", n)
    assert 0.1 * n <= ok.sum() <= 0.9 * n, ok.sum()
    m = L.N_CERTIFIED_STEER                   # the steer-mode subset the GPU file compares with the restatement, at threshold 0.01
    ok = reference_continuous(sm, orc, s[:m], g[:m], L.MAX_DISTANCE["steer"], mode="steer", threshold=0.01)[0]
    print(name, "certified valid, steer", int(ok.sum()), "of", m)
    assert 0.1 * m <= ok.sum() <= 0.9 * m, ok.sum()


@pytest.mark.parametrize("name", L.SPLINE_CASES)
def test_trajectories_are_neither_all_free_nor_all_colliding(name, tmp_path):
    """Valid share of the 64 trajectories under the sampled check, degree 3 / 5; valid of the first 10 under the certified check;
    and, measured once with the restatement on all 64 (a minute per degree on k32d, so not repeated here: the GPU file holds the
    10-90 % bar on all 64 with the device's verdicts, which its first 10 tie to the restatement), valid of all 64:

        k16   0.42 0.45   3 4   23 16
        k32d  0.53 0.42   2 2   11  7
        tree  0.38 0.41   3 5   21 20
    """
    from numbotics_amd.planning import unit_knots
    from spline_ref import reference_splines
    from spline_continuous_ref import reference_spline_continuous
    arm, chain, sm = _model(name, tmp_path)
    orc = Oracle(sm)
    n = L.N_CERTIFIED_SPLINES
    for k, n_ctrl in L.SPLINE_SHAPES:
        c = L.splines(name, chain, n_ctrl)
        kn = unit_knots(n_ctrl, k)
        ok = reference_splines(orc, c, kn, k, L.SPLINE_RESOLUTION)[0]
        cert = reference_spline_continuous(sm, orc, c[:n], kn, k)[0]
        print(name, k, "sampled valid", ok.mean(), "certified valid", int(cert.sum()), "of", n)
        assert 0.1 <= ok.mean() <= 0.9, (k, ok.mean())
        assert 0.1 * n <= cert.sum() <= 0.9 * n, (k, cert.sum())


def _kin_inputs(name, tmp_path, n=64):
    arm, chain, sm = _model(name, tmp_path)
    return sm.kin, chain, L.sample(chain, n, 113)


@pytest.mark.parametrize("name", L.NAMES)
def test_oracle_fk_against_long_double(name, tmp_path):
    """Bar: 1e-12 max-abs on the 3x4 block, the bar of the golden FK vectors.  Measured maxima over first / middle / last frame
    and 64 configurations over the full limits: k9 4.9e-16, k16 4.6e-16, k18 6.4e-16, k24 6.8e-16, k25 8.8e-16, k32s 8.4e-16,
    k32d 1.1e-15, tree 9.1e-16."""
    kin, chain, q = _kin_inputs(name, tmp_path)
    orc = Oracle(kin)
    worst = 0.0
    for frame in L.probe_frames(kin):
        T = orc.fk(q, frame)
        for b in range(q.shape[0]):
            ref = L.fk_longdouble(kin, q[b], frame)
            worst = max(worst, float(np.abs(T[b, :3, :4] - ref[:3, :4]).max()))
            assert np.array_equal(T[b, 3], [0.0, 0.0, 0.0, 1.0])
    print(name, "fk max abs deviation", worst)
    assert worst < 1e-12


@pytest.mark.parametrize("name", L.NAMES)
def test_oracle_jacobian_against_long_double(name, tmp_path):
    """Bar: 1e-12 max-abs over the 6 x n_q entries.  Measured maxima (same frames and configurations as the FK test): k9 5.4e-16,
    k16 4.1e-16, k18 6.1e-16, k24 7.0e-16, k25 9.5e-16, k32s 9.6e-16, k32d 9.6e-16, tree 1.1e-15.  Columns of joints off the
    path are exact zeros."""
    kin, chain, q = _kin_inputs(name, tmp_path)
    orc = Oracle(kin)
    worst = 0.0
    for frame in L.probe_frames(kin):
        J = orc.jacobian(q, frame)
        on_path = {int(kin.joint_qidx[k]) for k in kin.frames[frame].path}
        off = [c for c in range(kin.n_q) if c not in on_path]
        assert not J[:, :, off].any()
        for b in range(q.shape[0]):
            worst = max(worst, float(np.abs(J[b] - L.jacobian_longdouble(kin, q[b], frame)).max()))
    print(name, "jacobian max abs deviation", worst)
    assert worst < 1e-12


# largest |jacobian_longdouble - central differences of fk_longdouble| over the position rows of the aligned-axes robot (step 1e-6
# in long double, 16 configurations, first / middle / last frame): the reference pair's own disagreement, measured on the CPU as
# 2.19e-13 (at this step the truncation error h^2 / 6 times the third derivative and the rounding error 2^-64 |p| / h are both
# of that size)
FD_REFERENCE_PAIR = 2.2e-13
FD_STEP = 1e-6


def test_oracle_jacobian_against_central_differences(tmp_path):
    """On a 20-joint robot with exact unit axes the model's rotation is a rotation, so the position rows are the derivative of FK.
    Bar: 100 x FD_REFERENCE_PAIR = 2.2e-11; the oracle's rows measured 2.19e-13 from the differences (the same as the pair: its
    own error, 1e-15, is far below the error of the differences)."""
    arm, chain = L.aligned_robot(tmp_path)
    kin = arm._kin
    assert kin.n_joints == L.ALIGNED["joints"]
    unit = np.sort(np.abs(kin.joint_axis), axis=1)
    assert np.array_equal(unit, np.tile([0.0, 0.0, 1.0], (kin.n_joints, 1)))
    q = L.sample(chain, 16, 127)
    orc = Oracle(kin)
    h = L.LD(FD_STEP)
    pair = got = 0.0
    for frame in L.probe_frames(kin):
        J = orc.jacobian(q, frame)
        for b in range(q.shape[0]):
            fd = np.zeros((3, kin.n_q), dtype=L.LD)
            for j in range(kin.n_q):
                qp, qm = q[b].astype(L.LD), q[b].astype(L.LD)
                qp[j] += h
                qm[j] -= h
                fd[:, j] = (L.fk_longdouble(kin, qp, frame)[:3, 3] - L.fk_longdouble(kin, qm, frame)[:3, 3]) / (2 * h)
            pair = max(pair, float(np.abs(L.jacobian_longdouble(kin, q[b], frame)[:3] - fd).max()))
            got = max(got, float(np.abs(J[b, :3] - fd).max()))
    print("reference pair", pair, "oracle vs differences", got)
    assert pair < 10 * FD_REFERENCE_PAIR, "the reference pair disagrees far more than when the bar was written down"
    assert got < 100 * FD_REFERENCE_PAIR


@pytest.mark.parametrize("name,path_len", L.IK_CASES, ids=[c for c, _ in L.IK_CASES])
def test_oracle_ik_on_long_chains(name, path_len, tmp_path):
    """256 problems per case, targets from FK of random configurations, starts within +-0.1, defaults otherwise.  Bars: success
    >= 0.9, position error of the solved ones < 1e-6 through fk_longdouble.  Measured: success 1.0 on all four; steps at most 11
    (k9), 6 (k16), 5 (k24), 7 (k32s, 12-joint path); position error at most 9.0e-7."""
    arm, chain, sm = _model(name, tmp_path)
    kin = sm.kin
    orc = Oracle(kin)
    frame = L.ik_frame(kin, path_len)
    assert len(kin.frames[frame].path) == (kin.n_joints if path_len is None else path_len)
    pose, q0 = L.ik_problems(orc, chain, frame, 256)
    ok, q, nrm, it = orc.ik(pose, q0, frame)
    err = max(float(np.abs(L.fk_longdouble(kin, q[b], frame)[:3, 3] - pose[b, :3, 3]).max()) for b in np.flatnonzero(ok))
    print(name, "ik success", ok.mean(), "max steps", it.max(), "max position error", err)
    assert ok.mean() >= 0.9
    assert err < 1e-6
    assert (nrm[ok] < 1e-6).all()
    on_path = {int(kin.joint_qidx[k]) for k in kin.frames[frame].path}
    off = [c for c in range(kin.n_q) if c not in on_path]
    assert np.array_equal(q[:, off], q0[:, off])
