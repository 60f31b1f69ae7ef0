"""Certified continuous B-spline checks on the device (nbk_spline_continuous_batch: k_spline_ca_init, k_spline_ca<K>,
k_ca_final): valid / t_free / status bit-identical to the NumPy + oracle restatement (tests/spline_continuous_ref.py), the
two-point linear spline against the edge path, soundness on the thin plate and against the sampled check, graph capture, degenerate
input, other descriptors and the C layer's error codes.  Needs a real MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd.planning import unit_bspline, unit_knots
from numbotics_amd.scenes import build_scene
from test_gpu_parity import torch_cuda      # noqa: F401  (fixture)
from continuous_ref import random_edges, thin_plate_scene, FREE, DEGENERATE
from spline_ref import random_splines
from spline_continuous_ref import dense_min_distance, reference_spline_continuous, spline_from_edges

SCENES = [("c2", True), ("c2", False), ("c3", True), ("c3", False), ("c2m", True), ("c2m", False)]
IDS = [f"{s}-{'bullet' if m else 'sharp'}" for s, m in SCENES]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_same(got, ref, what):
    v, tf, st = got
    rv, rtf, rst = ref[:3]
    assert np.array_equal(st, rst), f"{what}: status differs on {np.nonzero(st != rst)[0][:10]}"
    assert np.array_equal(v, rv), f"{what}: valid differs on {np.nonzero(v != rv)[0][:10]}"
    assert np.array_equal(_bits(tf), _bits(rtf)), f"{what}: t_free differs on {np.nonzero(_bits(tf) != _bits(rtf))[0][:10]}"


def _free_q(orc, chain, seed):
    q = random_splines(chain, 2000, 2, seed)[:, 0] * 0.3
    return q[~orc.validity(q)][0]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("scene,margins", SCENES, ids=IDS)
def test_bit_parity_with_the_restatement(fresh_world, scene, margins, k, torch_cuda):
    arm, chain, obs = build_scene(scene, bullet_margins=margins)
    sm = arm.scene_model()
    orc = Oracle(sm)
    _, dev = arm._scene_device()
    free = _free_q(orc, chain, 5)
    thresholds = (0.0, 0.01, -0.002) if not margins else (0.0, 0.01, 0.0)
    n_free = n_other = 0
    for i, n in enumerate(sorted({k + 1, (k + 13) // 2, 10})):
        c = random_splines(chain, 24, n, 1000 * k + n, near=free, spread=(0.05, 0.3)[i % 2])
        c[1, 1] = c[1, 0]                                               # a leg of zero length
        thr = thresholds[i % 3]
        got = dev.spline_continuous(c, unit_knots(n, k), k, threshold=thr)
        _assert_same(got, reference_spline_continuous(sm, orc, c, unit_knots(n, k), k, threshold=thr), f"{scene} k={k} n={n} thr={thr}")
        n_free += int(got[0].sum())
        n_other += int((~got[0]).sum())
    assert n_free > 0 and n_other > 0


def test_repeated_knots_and_few_iterations(fresh_world, torch_cuda):
    """Knot vectors with empty interior spans (crossed without an evaluation), and max_iter / slack other than the defaults."""
    arm, chain, obs = build_scene("c3", bullet_margins=False)
    sm = arm.scene_model()
    orc = Oracle(sm)
    _, dev = arm._scene_device()
    free = _free_q(orc, chain, 9)
    kn = np.array([0.0, 0.0, 0.0, 0.0, 0.25, 0.25, 0.6, 0.6, 0.6, 1.0, 1.0, 1.0, 1.0])
    c = random_splines(chain, 40, 9, 77, near=free, spread=0.1)
    for max_iter, slack in ((64, 1e-6), (5, 1e-6), (64, 1e-3)):
        got = dev.spline_continuous(c, kn, 3, max_iter=max_iter, slack=slack)
        _assert_same(got, reference_spline_continuous(sm, orc, c, kn, 3, max_iter=max_iter, slack=slack), f"{max_iter} {slack}")


@pytest.mark.parametrize("scene,margins", [("c2", True), ("c2", False), ("c3", True), ("c3", False)],
                         ids=["c2-bullet", "c2-sharp", "c3-bullet", "c3-sharp"])
def test_linear_spline_is_the_edge_path(fresh_world, scene, margins, torch_cuda):
    from numbotics_amd.planning.sampling_based import ConnectorParams, ContinuousConnector
    arm, chain, obs = build_scene(scene, bullet_margins=margins)
    _, dev = arm._scene_device()
    s, g = random_edges(chain, 600, 13, scale=0.3)
    g[:20] = s[:20]                                                   # degenerate: zero length
    g[20:40] = s[20:40] + 1e-9                                        # degenerate: below float32 eps
    s[40, 2] = np.nan
    g[41, 0] = np.inf
    ctrl = np.stack((s, g), axis=1)
    ok, _, tf, st = ContinuousConnector(ConnectorParams(max_distance=10.0, arm=arm)).certify_batch(s, g)
    _assert_same(ContinuousConnector(ConnectorParams(max_distance=10.0, arm=arm)).validate_trajectories(ctrl, degree=1),
                 (ok, tf, st), f"{scene} connector")
    assert (st[:42] == DEGENERATE).all() and 0 < ok.sum() < 600
    for thr in (0.01, -0.002):
        ok, _, tf, st = dev.edge_continuous(s, g, 10.0, threshold=thr)
        _assert_same(dev.spline_continuous(ctrl, unit_knots(2, 1), 1, threshold=thr), (ok, tf, st), f"{scene} thr={thr}")


def test_thin_plate_is_not_stepped_over(fresh_world, torch_cuda):
    from numbotics_amd.planning.sampling_based import ConnectorParams, ContinuousConnector, DiscreteConnector
    arm, chain, obs = thin_plate_scene()
    sm = arm.scene_model()
    orc = Oracle(sm)
    s, g = random_edges(chain, 400, 5, scale=0.4)
    keep = ~orc.validity(s) & ~orc.validity(g)
    c = spline_from_edges(s[keep], g[keep])
    kn = unit_knots(4, 3)
    cp = ConnectorParams(resolution=0.05, max_distance=10.0, arm=arm)
    disc = DiscreteConnector(cp).validate_trajectories(c, degree=3)[0]
    hits = [e for e in np.nonzero(disc)[0] if dense_min_distance(orc, c[e], kn, 3) <= 0.0]
    assert hits, "no spline crosses the plate between two samples"
    cc = ContinuousConnector(cp)
    valid, t_free, status = cc.validate_trajectories(c, degree=3)
    assert not valid[hits].any()
    assert (status[hits] != FREE).all()
    one = unit_bspline(c[hits[0]], degree=3)
    assert cc.validate_trajectory(one)[0] is False and DiscreteConnector(cp).validate_trajectory(one)[0] is True
    for e in np.nonzero(valid)[0][:80]:
        assert dense_min_distance(orc, c[e], kn, 3) > 0.0, f"spline {e} certified free but a dense sample touches"
    _assert_same((valid[:40], t_free[:40], status[:40]), reference_spline_continuous(sm, orc, c[:40], kn, 3), "thin plate")


def _planner_splines(chain, S, seed, n=8):
    """Smoothings of planner-like paths: n control points along a short edge, each moved by up to 0.05 rad."""
    s, g = random_edges(chain, S, seed, scale=0.25)
    rng = np.random.default_rng(seed + 1)
    return spline_from_edges(s, g, n) + rng.uniform(-0.05, 0.05, (S, n, chain.dof))


@pytest.mark.parametrize("scene", ["c2", "c3"])
def test_free_is_a_subset_of_the_sampled_check(fresh_world, scene, torch_cuda):
    arm, chain, obs = build_scene(scene)
    _, dev = arm._scene_device()
    c = _planner_splines(chain, 2000, 41)
    kn = unit_knots(8, 3)
    v, tf, st = dev.spline_continuous(c, kn, 3)
    sv, _, ns = dev.spline_validity(c, kn, 3, 0.001)
    assert v.sum() > 200
    assert not (v & ~sv).any(), f"{int((v & ~sv).sum())} splines certified free fail the sampled check"
    assert (st[ns == 0] == DEGENERATE).all() and (ns[st == DEGENERATE] == 0).all()


def test_graph_capture_replays_the_direct_call(fresh_world, torch_cuda):
    torch = torch_cuda
    arm, chain, obs = build_scene("c2")
    _, dev = arm._scene_device()
    c = torch.from_numpy(_planner_splines(chain, 3000, 9)).cuda()
    kn = torch.from_numpy(unit_knots(8, 3)).cuda()
    direct = [x.clone() for x in dev.spline_continuous(c, kn, 3)]
    assert 0 < int(direct[0].sum()) < 3000
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        dev.spline_continuous(c, kn, 3)                             # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = dev.spline_continuous(c, kn, 3)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(2):
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, direct):
            assert torch.equal(a, b) or (a.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64)))


def _nan_at_the_end(c):
    """Knots [0, 0, 1, 1, 1] and a NaN in the last control point of trajectory 9: the sampled path reaches it only at t = 1."""
    c = c.copy()
    c[9, 2] = np.nan
    return c, np.array([0.0, 0.0, 1.0, 1.0, 1.0])


def test_degenerate_input(fresh_world, torch_cuda):
    torch = torch_cuda
    arm, chain, obs = build_scene("c3")
    sm = arm.scene_model()
    orc = Oracle(sm)
    _, dev = arm._scene_device()
    free = _free_q(orc, chain, 3)
    c = random_splines(chain, 10, 5, 4, near=free, spread=0.05)
    c[1, 3, 2] = np.nan
    c[2] = free                                                         # every control point equal
    c[5, 0] = np.nan
    c[6, 4, 1] = np.inf
    c[7, 2, 0] = -np.inf
    kn = unit_knots(5, 3)
    v, tf, st = dev.spline_continuous(c, kn, 3)
    _assert_same((v, tf, st), reference_spline_continuous(sm, orc, c, kn, 3), "degenerate")
    assert (st[[1, 2, 5, 6, 7]] == DEGENERATE).all() and not v[[1, 2, 5, 6, 7]].any() and np.isnan(tf[[1, 2, 5, 6, 7]]).all()
    assert (st[[0, 3, 4, 8, 9]] != DEGENERATE).all()
    ns = dev.spline_validity(c, kn, 3, 0.02)[2]
    assert (st[ns == 0] == DEGENERATE).all()
    c1, kn1 = _nan_at_the_end(random_splines(chain, 12, 3, 6, near=free, spread=0.05))
    v, tf, st = dev.spline_continuous(c1, kn1, 1)
    assert st[9] == DEGENERATE and dev.spline_validity(c1, kn1, 1, 0.02)[2][9] > 0
    _assert_same((v, tf, st), reference_spline_continuous(sm, orc, c1, kn1, 1), "NaN at the end")
    # knots on the device that break the rules: every trajectory is degenerate
    c2 = random_splines(chain, 6, 6, 8, near=free, spread=0.05)
    good = unit_knots(6, 3)
    for bad in (good * 2.0, good - 0.25, np.where(good == 1.0, np.nan, good), np.concatenate((good[:5], [0.2], good[6:])),
                np.where(good == 0.0, -np.inf, good)):
        v, tf, st = dev.spline_continuous(c2, torch.from_numpy(bad).cuda(), 3)
        assert (st == DEGENERATE).all() and not v.any() and np.isnan(tf).all(), bad
    assert (dev.spline_continuous(c2, good, 3)[2] != DEGENERATE).all()


def test_other_descriptors(fresh_world, torch_cuda, tmp_path):
    from numbotics_amd.physics import GraphChain
    from numbotics_amd.robots import Arm
    from random_scenes import random_urdf, random_obstacles
    from numbotics_amd.engine import DeviceModel
    rng = np.random.default_rng(124)
    chain = GraphChain.from_urdf(random_urdf(rng, 36, str(tmp_path / "big.urdf"), max_back=1))
    arm = Arm(chain)
    obs = random_obstacles(rng, 3)      # noqa: F841  (the world holds weak references)
    sm = arm.scene_model()
    assert sm.n_rshapes >= 25
    orc = Oracle(sm)
    _, dev = arm._scene_device()
    c = random_splines(chain, 24, 6, 9, near=np.zeros(chain.dof), spread=0.1)
    for k in (1, 3):
        _assert_same(dev.spline_continuous(c, unit_knots(6, k), k), reference_spline_continuous(sm, orc, c, unit_knots(6, k), k),
                     f"big robot k={k}")
    # the same robot without any pair: every non-degenerate trajectory is FREE at 1
    sm0 = arm.scene_model(pairs=[])
    assert sm0.n_pairs == 0
    dev0 = DeviceModel(sm0)
    c0 = c.copy()
    c0[3, 2, 4] = np.inf
    v, tf, st = dev0.spline_continuous(c0, unit_knots(6, 5), 5)
    _assert_same((v, tf, st), reference_spline_continuous(sm0, Oracle(sm0), c0, unit_knots(6, 5), 5), "no pairs")
    assert st[3] == DEGENERATE and v.sum() == 23 and (tf[v] == 1.0).all()


def test_error_codes(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd import _lib
    arm, chain, obs = build_scene("c2")
    _, dev = arm._scene_device()
    lib = _lib.load()
    S, n, k = 4, 6, 3
    ctrl = torch.from_numpy(random_splines(chain, S, n, 2) * 0.2).cuda()
    kn = torch.from_numpy(unit_knots(n, k)).cuda()
    v = torch.empty((S,), dtype=torch.uint8, device="cuda")
    tf = torch.empty((S,), dtype=torch.float64, device="cuda")
    stt = torch.empty((S,), dtype=torch.int32, device="cuda")

    def call(S=S, n=n, k=k, knots=kn.data_ptr(), thr=0.0, it=64, slack=1e-6, ctrl_p=ctrl.data_ptr(), valid=v.data_ptr(),
             t_free=tf.data_ptr(), status=stt.data_ptr(), h=dev._h):
        return lib.nbk_spline_continuous_batch(h, ctrl_p, S, n, k, knots, thr, it, slack, valid, t_free, status, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert (stt.cpu().numpy() != DEGENERATE).all()
    nan = float("nan")
    for kw in (dict(it=0), dict(slack=-1.0), dict(slack=nan), dict(thr=nan), dict(k=0), dict(k=6, n=8), dict(n=3),
               dict(n=70000), dict(S=-1), dict(knots=None), dict(ctrl_p=None), dict(valid=None), dict(t_free=None),
               dict(status=None), dict(h=None)):
        assert call(**kw) == -1, kw
    assert call(S=0, ctrl_p=None, valid=None, t_free=None, status=None) == 0
    with pytest.raises(_lib.NbkError):
        dev.spline_continuous(ctrl, kn, k, max_iter=0)
