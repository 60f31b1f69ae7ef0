"""Moving world bodies on the device (nbk_model_create_movable, nbk_model_set_world_poses*, k_world_update, k_world_guard): after
every update the whole pipeline equals the oracle at the new poses AND a freshly created ordinary descriptor at those poses, bit for
bit; no table survives an update; an update is a graph node; bad poses force every verdict; the Arm keeps its descriptor through
obstacle moves.  Needs a real MI355X."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd import _lib
from numbotics_amd._lib import debug_option, NbkError, CA_UNDECIDED
from numbotics_amd.engine import DeviceModel, world_reach_bounds
from numbotics_amd.planning import unit_knots
from numbotics_amd.scenes import sample_q
from test_gpu_parity import torch_cuda      # noqa: F401  (fixture)
from test_world_poses_host import world_scene, random_rotation, robot_reach, SH_PLANE
from continuous_ref import reference_continuous, random_edges
from spline_ref import random_splines, reference_splines
from spline_continuous_ref import reference_spline_continuous

THRESHOLDS = (0.0, 1e-6, 0.01, -0.002)          # the four narrowphase builds
BATCHES = (1, 63, 4096, 1 << 17)                # below and above the 65 536 rows at which the per-robot broadphase is compiled
RES, MAXD = 0.05, 10.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} / {b.shape}"
    if a.dtype.kind == "f":
        bad = np.nonzero(bits(a).reshape(-1) != bits(b).reshape(-1))[0]
    else:
        bad = np.nonzero(a.reshape(-1) != b.reshape(-1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} entries differ, first at {bad[:8]}"


def unpack(words, B):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:B].astype(bool)


def pose_sets(sm, seed):
    """K = 8 pose sets (W, 12) and the radius they stay inside: the scene's own; a shuffle near the robot; EVERY obstacle out of
    reach; back near the robot (the reachable-world list has to come back); that with one obstacle moved by 1e-9 m; three more
    shuffles.  Planes keep their rotation (their normal is a shape parameter) and move their point."""
    rng = np.random.default_rng(seed)
    reach = robot_reach(sm)
    W = sm.n_wshapes
    P0 = sm.wshape_pose.reshape(W, 3, 4)

    def unit():
        d = rng.normal(size=3)
        return d / np.linalg.norm(d)

    def near(spread):
        P = P0.copy()
        for w in range(W):
            d = unit()
            if sm.wshape_type[w] == SH_PLANE:
                n = sm.wshape_param[w, :3]
                P[w, :, 3] = P0[w, :, 3] - n * rng.uniform(0.0, 0.06) + (d - n * (d @ n)) * spread      # (never up into the base link)
            else:
                P[w, :, :3] = random_rotation(rng)
                P[w, :, 3] = P0[w, :, 3] + d * spread * rng.uniform()
        return P

    def far():
        P = P0.copy()
        for w in range(W):
            if sm.wshape_type[w] == SH_PLANE:
                P[w, :, 3] = -sm.wshape_param[w, :3] * 2.5 * reach
            else:
                P[w, :, :3] = random_rotation(rng)
                P[w, :, 3] = unit() * 2.5 * reach
        return P

    sets = [P0.copy(), near(0.2), far(), near(0.3)]
    nudged = sets[3].copy()
    nudged[W - 1, 0, 3] += 1e-9
    sets += [nudged, near(0.15), near(0.4), near(0.25)]
    return [np.ascontiguousarray(P.reshape(W, 12)) for P in sets], 3.0 * reach


def check_validity_forms(torch, dev, qt, B, thr, ws, ref, what):
    """bits and bytes, the descriptor's own workspace and the caller's."""
    same(dev.validity(qt[:B], thr).cpu().numpy(), ref[:B], f"{what} bytes")
    same(unpack(dev.validity(qt[:B], thr, packed=True).cpu().numpy(), B), ref[:B], f"{what} bits")
    same(dev.validity(qt[:B], thr, workspace=ws).cpu().numpy(), ref[:B], f"{what} bytes, caller's workspace")
    same(unpack(dev.validity(qt[:B], thr, packed=True, workspace=ws).cpu().numpy(), B), ref[:B], f"{what} bits, caller's workspace")


SCENES = ["c2", "c3", "c5m", "plane", "tree"]


@pytest.mark.parametrize("margins", [True, False], ids=["bullet", "sharp"])
@pytest.mark.parametrize("scene", SCENES)
def test_parity_after_moves(fresh_world, scene, margins, torch_cuda):
    torch = torch_cuda
    arm, chain, obs = world_scene(scene, bullet_margins=margins)
    sm = arm.scene_model()
    S = sm.n_rshapes
    assert sm.n_wshapes > 0 and (sm.pair_b >= S).any(), "a scene without robot-world pairs tests nothing here"
    sets, radius = pose_sets(sm, 100 + SCENES.index(scene))
    assert len(sets) == 8
    dev = DeviceModel(sm, movable=True, world_radius=radius)
    handle = dev._h.value
    BIG = BATCHES[-1]
    q = sample_q(chain, BIG, seed=11)
    qt = torch.from_numpy(q).cuda()
    ws = torch.empty((max(dev.validity_workspace_bytes(BIG), 64),), dtype=torch.uint8, device="cuda")
    NB, E, NS = 1024, 192, 32
    NE, SPL = 6, slice(NS // 2 - 2, NS // 2 + 2)      # what the restatements of the certified checks see: 6 edges; 2 spread + 2 clustered splines
    s, g = random_edges(chain, E, 7, scale=0.3)
    free = q[:4096][~Oracle(sm).validity(q[:4096], 0.0)][0]
    n_ctrl, deg = 6, 3
    ctrl = random_splines(chain, NS, n_ctrl, 9, near=free, spread=0.2)
    kn = unit_knots(n_ctrl, deg)
    rng = np.random.default_rng(5)
    items = np.stack((rng.integers(0, NB, 2048), rng.integers(0, sm.n_pairs, 2048)), axis=1).astype(np.int32)
    mixed = 0
    for k, P in enumerate(sets):
        if k % 2 == 0:
            dev.set_world_poses(torch.from_numpy(P).cuda())                 # the device entry, on the current stream
        else:
            dev.set_world_poses(P.reshape(-1, 3, 4))                        # the host entry (pinned staging)
        assert dev.world_status() == 0
        smk = dataclasses.replace(sm, wshape_pose=P)
        orc = Oracle(smk)
        fresh = DeviceModel(smk)
        tag = f"{scene} {'bullet' if margins else 'sharp'} P_{k}"
        if k == 2:                                                          # every obstacle is out of reach, by the bound itself
            b = world_reach_bounds(sm, P)
            assert np.all(b[np.isfinite(b)] > 0.1)
        # -- validity: the full cross product
        for thr in THRESHOLDS:
            ref = orc.validity(q, thr, nthreads=8)
            mixed += 0.02 < ref.mean() < 0.98
            for B in BATCHES:
                check_validity_forms(torch, dev, qt, B, thr, ws, ref, f"{tag} thr={thr} B={B}")
                same(fresh.validity(qt[:B], thr).cpu().numpy(), ref[:B], f"{tag} thr={thr} B={B} fresh descriptor")
                if B == BIG:
                    dev.validity(qt[:B], thr)
                    if fresh.broad_kernel_used() == 2:                      # the per-robot broadphase serves the movable one too
                        assert dev.broad_kernel_used() == 2, tag
        for thr in (0.0, -0.002):
            ref = orc.validity(q[:4096], thr, nthreads=8)
            with debug_option("f64_broad", 1):
                same(dev.validity(qt[:4096], thr).cpu().numpy(), ref, f"{tag} thr={thr} float64 broadphase")
            with debug_option("two_kernel_min_b", 10 ** 9):
                same(dev.validity(qt[:4096], thr).cpu().numpy(), ref, f"{tag} thr={thr} fused kernel")
            with debug_option("no_reg_broad", 1):
                same(dev.validity(qt[:4096], thr).cpu().numpy(), ref, f"{tag} thr={thr} LDS broadphase")
            # -- the scalar host calls follow the update without the caller's help
            for i in range(6):
                assert dev.validity_scalar(q[i], thr) == bool(ref[i]), f"{tag} thr={thr} scalar {i}"
            # -- edges
            ev = orc.edge_validity(s, g, RES, MAXD, threshold=thr, nthreads=8)
            got = dev.edge_validity(torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda(), RES, MAXD, threshold=thr)
            fr = fresh.edge_validity(s, g, RES, MAXD, threshold=thr)
            for j, name in enumerate(("valid", "end", "n_samples")):
                same(got[j].cpu().numpy(), ev[j], f"{tag} thr={thr} edge {name}")
                same(fr[j], ev[j], f"{tag} thr={thr} edge {name}, fresh descriptor")
            for i in range(3):
                ok, end, ns = dev.edge_validity_scalar(s[i], g[i], RES, MAXD, threshold=thr)
                assert ok == bool(ev[0][i]) and ns == int(ev[2][i]), f"{tag} thr={thr} scalar edge {i}"
                same(end, ev[1][i], f"{tag} thr={thr} scalar edge {i} end")
            # -- certified edges and splines: the fresh descriptor on the full set, the NumPy + oracle restatements (the
            #    independent reference) on a fixed handful of edges / splines -- at every pose set and both thresholds
            ec = dev.edge_continuous(s, g, MAXD, threshold=thr)
            ef = fresh.edge_continuous(s, g, MAXD, threshold=thr)
            for j, name in enumerate(("valid", "end", "t_free", "status")):
                same(ec[j], ef[j], f"{tag} thr={thr} continuous edge {name}")
            sc = dev.spline_continuous(ctrl, kn, deg, threshold=thr)
            sf = fresh.spline_continuous(ctrl, kn, deg, threshold=thr)
            for j, name in enumerate(("valid", "t_free", "status")):
                same(sc[j], sf[j], f"{tag} thr={thr} continuous spline {name}")
            sv = dev.spline_validity(ctrl, kn, deg, RES, threshold=thr)
            rv = reference_splines(orc, ctrl, kn, deg, RES, threshold=thr)
            fv = fresh.spline_validity(ctrl, kn, deg, RES, threshold=thr)
            for j, name in enumerate(("valid", "t_hit", "n_samples")):
                same(sv[j], rv[j], f"{tag} thr={thr} sampled spline {name}")
                same(fv[j], rv[j], f"{tag} thr={thr} sampled spline {name}, fresh descriptor")
            r = reference_continuous(smk, orc, s[:NE], g[:NE], MAXD, threshold=thr)
            for j, name in enumerate(("valid", "end", "t_free", "status")):
                same(ec[j][:NE], r[j], f"{tag} thr={thr} continuous edge {name} vs restatement")
            r = reference_spline_continuous(smk, orc, ctrl[SPL], kn, deg, threshold=thr)
            for j, name in enumerate(("valid", "t_free", "status")):
                same(sc[j][SPL], r[j], f"{tag} thr={thr} continuous spline {name} vs restatement")
        # -- distances
        d, idx = dev.closest(qt[:NB])
        dr, ir = orc.closest(q[:NB])
        same(d.cpu().numpy(), dr, f"{tag} closest distance")
        same(idx.cpu().numpy(), ir, f"{tag} closest pair")
        df, idf = fresh.closest(q[:NB])
        same(df, dr, f"{tag} closest distance, fresh descriptor")
        same(idf, ir, f"{tag} closest pair, fresh descriptor")
        pd, pw = dev.pair_distances(qt[:NB], witness=True)
        pdr, pwr, rows_r = orc.proximity_jacobian(q[:NB])
        same(pd.cpu().numpy(), pdr, f"{tag} pair distances")
        same(pw.cpu().numpy(), pwr, f"{tag} witnesses")
        same(dev.pair_distances(qt[:NB]).cpu().numpy(), pdr, f"{tag} pair distances without witnesses")
        fpd, fpw = fresh.pair_distances(q[:NB], witness=True)
        same(fpd, pdr, f"{tag} pair distances, fresh descriptor")
        same(fpw, pwr, f"{tag} witnesses, fresh descriptor")
        rd, rw, rj = dev.pair_records(qt[:NB], items)
        same(rd.cpu().numpy(), pdr[items[:, 0], items[:, 1]], f"{tag} record distances")
        same(rw.cpu().numpy(), pwr[items[:, 0], items[:, 1]], f"{tag} record witnesses")
        same(rj.cpu().numpy(), rows_r[items[:, 0], items[:, 1]], f"{tag} record rows")
        fd, fw, fj = fresh.pair_records(q[:NB], items)
        same(rd.cpu().numpy(), fd, f"{tag} record distances, fresh descriptor")
        same(rw.cpu().numpy(), fw, f"{tag} record witnesses, fresh descriptor")
        same(rj.cpu().numpy(), fj, f"{tag} record rows, fresh descriptor")
        assert dev._h.value == handle and dev.world_status() == 0
        del fresh
    assert mixed >= 8, "the batch is (almost) all free or all colliding on most pose sets: the comparison proves little"


def test_no_stale_tables(fresh_world, torch_cuda):
    """Same threshold, same stream, same q, poses changed between two calls: the tables the validity path keeps per stream must
    not survive the update -- on the updating stream and on another one ordered after it by an event."""
    torch = torch_cuda
    arm, chain, obs = world_scene("c2")
    sm = arm.scene_model()
    dev = DeviceModel(sm, movable=True, world_radius=4.0)
    q = sample_q(chain, 4096, seed=1)
    qt = torch.from_numpy(q).cuda()
    Pa = sm.wshape_pose.copy()
    Pb = Pa.copy().reshape(-1, 3, 4)
    Pb[:, 0, 3] += 0.1
    Pb = Pb.reshape(-1, 12)
    ra = Oracle(sm).validity(q, 0.0)
    rb = Oracle(dataclasses.replace(sm, wshape_pose=Pb)).validity(q, 0.0)
    assert (ra != rb).sum() > 50                                            # a stale table is visible
    ta, tb = torch.from_numpy(Pa).cuda(), torch.from_numpy(Pb).cuda()
    for _ in range(3):                                                      # steady state: tables in place for this threshold
        same(dev.validity(qt, 0.0).cpu().numpy(), ra, "before the move")
    dev.set_world_poses(tb)
    same(dev.validity(qt, 0.0).cpu().numpy(), rb, "after the move, same stream")
    same(dev.validity(qt, 0.0).cpu().numpy(), rb, "after the move, same stream, tables reused")
    # the update on one stream, the check on another
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        for _ in range(2):
            m = dev.validity(qt, 0.0)                                       # s2 has tables for Pb now
        same(m.cpu().numpy(), rb, "second stream before the move")
    for Pt, ref in ((ta, ra), (tb, rb), (ta, ra)):
        s1.wait_stream(s2)                                                  # the update must not overtake s2's earlier checks
        with torch.cuda.stream(s1):
            dev.set_world_poses(Pt)
            done = torch.cuda.Event()
            done.record(s1)
        with torch.cuda.stream(s2):
            s2.wait_event(done)
            m = dev.validity(qt, 0.0)
        s2.synchronize()
        same(m.cpu().numpy(), ref, "update on one stream, check on another")
    torch.cuda.synchronize()


def test_update_and_checks_in_one_graph(fresh_world, torch_cuda):
    """One captured graph: set_world_poses(P) + validity + edge_validity; replayed with P overwritten in place."""
    torch = torch_cuda
    arm, chain, obs = world_scene("c3")
    sm = arm.scene_model()
    sets, radius = pose_sets(sm, 42)
    dev = DeviceModel(sm, movable=True, world_radius=radius)
    B, E = 20000, 500
    q = sample_q(chain, B, seed=5)
    s, g = random_edges(chain, E, 8, scale=0.3)
    qt, st, gt = (torch.from_numpy(a).cuda() for a in (q, s, g))
    Pt = torch.from_numpy(sets[0]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev.set_world_poses(Pt)                                             # this stream's scratch is allocated outside the capture
        dev.validity(qt, 0.0)
        dev.edge_validity(st, gt, RES, MAXD)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            dev.set_world_poses(Pt)
            mask = dev.validity(qt, 0.0)
            valid, end, ns = dev.edge_validity(st, gt, RES, MAXD)
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 3, 6):
        Pt.copy_(torch.from_numpy(sets[k]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        orc = Oracle(dataclasses.replace(sm, wshape_pose=sets[k]))
        same(mask.cpu().numpy(), orc.validity(q, 0.0, nthreads=8), f"replay at P_{k}: validity")
        ev = orc.edge_validity(s, g, RES, MAXD, nthreads=8)
        same(valid.cpu().numpy(), ev[0], f"replay at P_{k}: edges")
        same(end.cpu().numpy(), ev[1], f"replay at P_{k}: edge ends")
        same(ns.cpu().numpy(), ev[2], f"replay at P_{k}: edge samples")
    # direct calls after the replays, on another stream, see the last replay's poses (no table is trusted any more)
    same(dev.validity(qt, 0.0).cpu().numpy(), Oracle(dataclasses.replace(sm, wshape_pose=sets[6])).validity(q, 0.0, nthreads=8),
         "direct call after the replays")


@pytest.mark.parametrize("margins", [True, False], ids=["bullet", "sharp"])
def test_bad_poses_force_every_verdict(fresh_world, margins, torch_cuda):
    torch = torch_cuda
    arm, chain, obs = world_scene("c2", bullet_margins=margins)
    sm = arm.scene_model()
    q = sample_q(chain, 4096, seed=1)
    good = sm.wshape_pose.copy()
    ref = Oracle(sm).validity(q, 0.0)
    assert 0.05 < 1.0 - ref.mean() < 0.95, "all colliding would prove nothing"
    radius = 3.0
    dev = DeviceModel(sm, movable=True, world_radius=radius)
    qt = torch.from_numpy(q).cuda()
    s, g = random_edges(chain, 64, 7, scale=0.3)
    ctrl = random_splines(chain, 16, 6, 9, near=q[~ref][0], spread=0.1)
    kn = unit_knots(6, 3)
    items = np.array([[0, 0], [5, 1], [17, sm.n_pairs - 1]], dtype=np.int32)
    nan_pose = good.copy()
    nan_pose[0, 5] = np.nan
    far_pose = good.copy().reshape(-1, 3, 4)
    far_pose[0, :, 3] = np.array([2.0 * radius, 0.0, 0.0])
    far_pose = far_pose.reshape(-1, 12)

    def all_forced(what):
        assert dev.validity(qt, 0.0).cpu().numpy().all(), what
        words = dev.validity(qt[:4000], 0.0, packed=True).cpu().numpy()
        assert unpack(words, 4000).all(), what
        with debug_option("two_kernel_min_b", 10 ** 9):
            assert dev.validity(qt, 0.0).cpu().numpy().all(), what
        assert dev.validity_scalar(q[~ref][0], 0.0) is True, what
        ok, end, ns = dev.edge_validity(s, g, RES, MAXD)
        assert not ok.any(), what
        assert dev.edge_validity_scalar(s[0], g[0], RES, MAXD)[0] is False, what
        ok, end, tf, stt = dev.edge_continuous(s, g, MAXD)
        assert not ok.any() and np.isnan(tf).all() and (stt == CA_UNDECIDED).all(), what
        ok, tf, stt = dev.spline_continuous(ctrl, kn, 3)
        assert not ok.any() and np.isnan(tf).all() and (stt == CA_UNDECIDED).all(), what
        ok, th, ns = dev.spline_validity(ctrl, kn, 3, RES)
        assert not ok.any() and not np.isnan(th).any(), what
        d, idx = dev.closest(q[:256])
        assert np.isnan(d).all() and (idx == -1).all(), what
        d, w = dev.pair_distances(q[:256], witness=True)
        assert np.isnan(d).all() and np.isnan(w).all(), what
        d, w, j = dev.proximity_jacobian(q[:256])
        assert np.isnan(d).all() and np.isnan(w).all() and np.isnan(j).all(), what
        d, w, j = dev.pair_records(q[:256], items)
        assert np.isnan(d).all() and np.isnan(w).all() and np.isnan(j).all(), what

    def all_good(P, what):
        smk = dataclasses.replace(sm, wshape_pose=P)
        orc = Oracle(smk)
        assert dev.world_status() == 0, what
        same(dev.validity(qt, 0.0).cpu().numpy(), orc.validity(q, 0.0), what)
        same(dev.edge_validity(s, g, RES, MAXD)[0], orc.edge_validity(s, g, RES, MAXD)[0], what)
        fresh = DeviceModel(smk)
        for a, b in zip(dev.edge_continuous(s, g, MAXD), fresh.edge_continuous(s, g, MAXD)):
            same(a, b, what)
        for a, b in zip(dev.spline_continuous(ctrl, kn, 3), fresh.spline_continuous(ctrl, kn, 3)):
            same(a, b, what)
        d, idx = dev.closest(q[:256])
        dr, ir = orc.closest(q[:256])
        same(d, dr, what)
        same(idx, ir, what)
        same(dev.pair_distances(q[:256]), orc.pair_distances(q[:256]), what)

    all_good(good, "before any bad pose")
    moved = good.copy().reshape(-1, 3, 4)
    moved[:, 0, 3] += 0.1
    moved = moved.reshape(-1, 12)
    for bad, code, entry in ((nan_pose, 2, "device"), (far_pose, 1, "device"), (nan_pose, 2, "host"), (far_pose, 1, "host")):
        if entry == "device":
            dev.set_world_poses(torch.from_numpy(bad).cuda())
        else:
            dev.set_world_poses(bad)
        assert dev.world_status() == code
        all_forced(f"status {code} through the {entry} entry")
        assert dev.world_status() == code                                   # checks do not clear it
        dev.set_world_poses(torch.from_numpy(moved).cuda())                 # the next good update does
        all_good(moved, f"after status {code} ({entry} entry)")
        dev.set_world_poses(good)
        all_good(good, f"back at the scene's own poses after status {code}")
    # both at once: the non-finite pose wins
    both = far_pose.copy()
    both[0, 0] = np.inf
    dev.set_world_poses(torch.from_numpy(both).cuda())
    assert dev.world_status() == 2
    dev.set_world_poses(good)
    assert dev.world_status() == 0


def test_ordinary_descriptors_refuse_updates(fresh_world, torch_cuda):
    torch = torch_cuda
    arm, chain, obs = world_scene("c2")
    sm = arm.scene_model()
    plain = DeviceModel(sm)
    lib = _lib.load()
    P = torch.from_numpy(sm.wshape_pose).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.nbk_model_set_world_poses(plain._h, P.data_ptr(), st) == -4
    assert lib.nbk_model_set_world_poses_host(plain._h, sm.wshape_pose.ctypes.data) == -4
    with pytest.raises(NbkError):
        plain.set_world_poses(P)
    assert plain.world_status() == 0
    dev = DeviceModel(sm, movable=True)
    assert lib.nbk_model_set_world_poses(dev._h, None, st) == -1
    with pytest.raises(ValueError):
        dev.set_world_poses(P[:, :11].contiguous())
    with pytest.raises(ValueError):
        dev.set_world_poses(P.float())
    with pytest.raises(NbkError):
        DeviceModel(sm, movable=True, world_radius=0.5)                     # the cube's centre lies beyond it
    # a radius no larger than the scene's own extent leaves the float32 slack, and so the compiled broadphase, as they are
    q = torch.from_numpy(sample_q(chain, 1 << 17, seed=2)).cuda()
    tight = DeviceModel(sm, movable=True, world_radius=float(np.max(np.linalg.norm(sm.wshape_pose.reshape(-1, 3, 4)[:, :, 3], axis=1))))
    a, b = plain.validity(q, 0.0), tight.validity(q, 0.0)
    assert torch.equal(a, b) and plain.broad_kernel_used() == tight.broad_kernel_used()


def test_arm_keeps_its_descriptor(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.physics import GraphChain
    from numbotics_amd.robots import Arm
    from test_world_poses_host import TREE_URDF
    arm, chain, obs = world_scene("c3", movable_world=True)
    other = GraphChain.from_urdf(TREE_URDF)
    other.base_pose = np.array([[1.0, 0, 0, 0.55], [0, 1.0, 0, -0.35], [0, 0, 1.0, 0.0], [0, 0, 0, 1.0]])
    q = sample_q(chain, 4096, seed=3)
    qt = torch.from_numpy(q).cuda()
    _, dev = arm._scene_device()
    handle = dev._h.value
    rng = np.random.default_rng(8)
    changed = 0
    last = Oracle(arm.scene_model()).validity(q, 0.0)
    for i in range(32):
        cube = obs[i % len(obs)]
        cube.position = cube.position + rng.uniform(-0.08, 0.08, 3)
        got = arm.in_collision(qt)
        ref = Oracle(arm.scene_model()).validity(q, 0.0)
        same(got.cpu().numpy(), ref, f"move {i}")
        changed += int((ref != last).sum())
        last = ref
        _, d = arm._scene_device()
        assert d is dev and d._h.value == handle
    assert changed > 100
    # the other chain's links are obstacles of this arm: its configuration moves them
    for i in range(4):
        qo = other.configuration
        qo[: min(3, len(qo))] += 0.2
        other.configuration = qo
        same(arm.in_collision(q), Oracle(arm.scene_model()).validity(q, 0.0), f"other chain, move {i}")
        assert arm._scene_device()[1]._h.value == handle
    # device-side poses: body poses composed with the constant shape locals on the device
    L = torch.from_numpy(arm.obstacle_shape_locals()).cuda()
    sm = arm.scene_model()
    rows = arm.obstacle_shape_index(obs[0])
    assert len(rows) == 1
    body = obs[0].pose.copy()
    body[:3, 3] += np.array([0.05, -0.02, 0.03])
    poses = sm.wshape_pose.copy().reshape(-1, 3, 4)
    shifted = (torch.from_numpy(body).cuda().unsqueeze(2) * L[rows[0]].unsqueeze(0)).sum(dim=1)     # body pose @ shape local, on the device
    poses[rows[0]] = shifted[:3, :].cpu().numpy()
    full = torch.from_numpy(poses).cuda()
    arm.set_obstacle_poses(full)
    same(arm.in_collision(q), Oracle(dataclasses.replace(sm, wshape_pose=poses.reshape(-1, 12))).validity(q, 0.0), "set_obstacle_poses")
    assert arm._scene_device()[1]._h.value == handle
    obs[0].position = obs[0].position                                       # the Python objects applied last win again
    same(arm.in_collision(q), Oracle(arm.scene_model()).validity(q, 0.0), "python poses after device poses")
    assert arm._scene_device()[1]._h.value == handle


def test_bisection_graph_survives_a_move(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.planning.safe_sets import counter_example_bisection
    arm, chain, obs = world_scene("c3", movable_world=True)
    orc = Oracle(arm.scene_model())
    q = sample_q(chain, 3000, seed=12)
    hit = orc.validity(q, 0.0)
    centre = q[~hit][0]

    def both():
        pts = torch.from_numpy(q[Oracle(arm.scene_model()).validity(q, 0.0)][:300]).cuda()
        a = counter_example_bisection(arm, centre, pts, graph=True)
        b = counter_example_bisection(arm, centre, pts, graph=False)
        same(a.cpu().numpy(), b.cpu().numpy(), "graphed against un-graphed bisection")
        return a.cpu().numpy()
    before = both()
    graphs = dict(arm.__dict__.get("_bisection_graphs", {}))
    assert len(graphs) == 1
    obs[0].position = obs[0].position + np.array([-0.1, 0.05, 0.1])
    after = both()
    now = arm.__dict__["_bisection_graphs"]
    assert len(now) == 1 and list(now.values())[0] is list(graphs.values())[0], "the captured graph was rebuilt"
    assert before.shape != after.shape or not np.array_equal(before, after)
