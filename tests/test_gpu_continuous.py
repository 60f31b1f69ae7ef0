"""ContinuousConnector on the device (nbk_edge_continuous_batch, k_edge_ca): valid / end / t_free / status bit-identical to the
NumPy + oracle restatement of the loop (tests/continuous_ref.py), soundness against discrete checks at scale, PRM, the thin
plate, graph capture and the C layer's error codes.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd.scenes import build_scene
from test_gpu_parity import torch_cuda      # noqa: F401  (fixture)
from continuous_ref import (random_edges, reference_continuous, thin_plate_scene, tree_scene, dense_min_distance,
                            FREE, DEGENERATE)

SCENES = [("c2", True), ("c2", False), ("c3", True), ("c3", False), ("c2m", True), ("c2m", False), ("tree", True), ("tree", False)]


def _scene(name, margins):
    if name == "tree":
        return tree_scene()
    return build_scene(name, bullet_margins=margins)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_same(dev, ref, what):
    v, end, tf, st = dev
    rv, rend, rtf, rst = ref[:4]
    assert np.array_equal(v, rv), f"{what}: valid differs on {np.nonzero(v != rv)[0][:10]}"
    assert np.array_equal(st, rst), f"{what}: status differs on {np.nonzero(st != rst)[0][:10]}"
    assert np.array_equal(_bits(tf), _bits(rtf)), f"{what}: t_free differs on {np.nonzero(_bits(tf) != _bits(rtf))[0][:10]}"
    assert np.array_equal(_bits(end), _bits(rend)), f"{what}: end differs"


def _edge_set(chain, seed):
    """Edges of mixed length, two degenerate ones, and edges that move only the last joint (mu = 0 for most pairs)."""
    s, g = random_edges(chain, 40, seed, scale=0.35)
    s2, g2 = random_edges(chain, 8, seed + 1)                       # long: steer clips them
    distal = s[:6].copy()
    gd = distal.copy()
    gd[:, -1] += 0.4
    deg = s[:2].copy()
    return np.concatenate((s, s2, distal, deg)), np.concatenate((g, g2, gd, deg + 1e-9))


@pytest.mark.parametrize("scene,margins", SCENES, ids=[f"{s}-{'bullet' if m else 'sharp'}" for s, m in SCENES])
def test_bit_parity_with_the_reference_loop(fresh_world, scene, margins, torch_cuda):
    arm, chain, obs = _scene(scene, margins)
    sm = arm.scene_model()
    orc = Oracle(sm)
    _, dev = arm._scene_device()
    s, g = _edge_set(chain, 31)
    n_free = 0
    for thr in (0.0, 0.01, -0.002):
        for mode in ("connect", "steer"):
            maxd = 0.6 if mode == "steer" else 10.0
            dist = None if thr != 0.01 else np.linalg.norm(g - s, axis=1)
            got = dev.edge_continuous(s, g, maxd, mode=mode, threshold=thr, dist=dist)
            ref = reference_continuous(sm, orc, s, g, maxd, mode=mode, threshold=thr, dist=dist)
            _assert_same(got, ref, f"{scene} thr={thr} {mode}")
            assert (got[3][-2:] == DEGENERATE).all() and np.isnan(got[1][-2:]).all()
            n_free += int(got[0].sum())
            if mode == "steer":
                assert (ref[5] == FREE).any()
    assert n_free > 0


def test_subset_of_discrete_checks_at_scale(fresh_world, torch_cuda):
    from numbotics_amd.planning.sampling_based import ConnectorParams, ContinuousConnector, DiscreteConnector
    arm, chain, obs = build_scene("c3")
    s, g = random_edges(chain, 10000, 41, scale=0.25)
    params = ConnectorParams(resolution=1e-3, max_distance=10.0, arm=arm)
    cont = ContinuousConnector(params).connect_batch(s, g)
    disc = DiscreteConnector(params).connect_batch(s, g)
    assert cont.sum() > 1000
    assert not (cont & ~disc).any(), f"{int((cont & ~disc).sum())} edges certified free fail the discrete check"


def test_prm_accepts_a_subset(fresh_world, torch_cuda):
    from numbotics_amd.planning.sampling_based import (ConnectorParams, ContinuousConnector, DiscreteConnector, EuclideanSpace,
                                                       PlannerParams, PRM)
    arm, chain, obs = build_scene("c2")
    lim = np.asarray(chain.joint_limits, dtype=np.float64)
    lim = np.where(np.isfinite(lim), lim, np.sign(lim) * np.pi)
    space = EuclideanSpace(lim[:, 0], lim[:, 1])
    cp = ConnectorParams(resolution=0.05, max_distance=2.0, arm=arm)
    params = PlannerParams(max_iters=300, k_nearest=8, goal_bias=0.05)
    start, goal = np.zeros(chain.dof), np.full(chain.dof, 0.3)
    rng = np.random.default_rng(3)
    samples = [goal.copy() if rng.random() < params.goal_bias else rng.uniform(lim[:, 0], lim[:, 1]) for _ in range(params.max_iters)]
    edges, cands = {}, {}
    for name, conn in (("discrete", DiscreteConnector(cp)), ("continuous", ContinuousConnector(cp))):
        prm = PRM(space, conn, params)
        prm.add_start(start)
        prm.add_goal(goal)
        prm.plan(samples)
        edges[name] = {(int(a), int(b)) for a, b in prm.edges}
        cands[name] = prm.n_candidate_edges
    assert cands["discrete"] == cands["continuous"]
    assert edges["continuous"] and edges["continuous"] <= edges["discrete"]


def test_thin_plate_on_the_device(fresh_world, torch_cuda):
    from numbotics_amd.planning.sampling_based import ConnectorParams, ContinuousConnector, DiscreteConnector
    arm, chain, obs = thin_plate_scene()
    sm = arm.scene_model()
    orc = Oracle(sm)
    s, g = random_edges(chain, 400, 5, scale=0.4)
    keep = ~orc.validity(s) & ~orc.validity(g)
    s, g = s[keep], g[keep]
    cp = ConnectorParams(resolution=0.05, max_distance=10.0, arm=arm)
    disc = DiscreteConnector(cp).connect_batch(s, g)
    hits = [e for e in np.nonzero(disc)[0] if dense_min_distance(orc, s[e], g[e]) <= 0.0]
    assert hits
    cc = ContinuousConnector(cp)
    valid, _, _, status = cc.certify_batch(s, g)
    assert not valid[hits].any()
    assert cc.connect(s[hits[0]], g[hits[0]]) is None
    assert DiscreteConnector(cp).connect(s[hits[0]], g[hits[0]]) is not None
    _assert_same(cc.certify_batch(s[:64], g[:64]), reference_continuous(sm, orc, s[:64], g[:64], 10.0), "thin plate")


def test_graph_capture_replays_the_direct_call(fresh_world, torch_cuda):
    torch = torch_cuda
    arm, chain, obs = build_scene("c2")
    _, dev = arm._scene_device()
    s, g = random_edges(chain, 3000, 9, scale=0.3)
    st = torch.from_numpy(s).cuda()
    gt = torch.from_numpy(g).cuda()
    direct = [x.clone() for x in dev.edge_continuous(st, gt, 1.0)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        dev.edge_continuous(st, gt, 1.0)                           # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = dev.edge_continuous(st, gt, 1.0)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(2):
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, direct):
            assert torch.equal(a, b) or (a.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64)))


def test_error_codes(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd import _lib
    arm, chain, obs = build_scene("c2")
    _, dev = arm._scene_device()
    lib = _lib.load()
    E, nq = 4, chain.dof
    s = torch.zeros((E, nq), dtype=torch.float64, device="cuda")
    g = torch.ones((E, nq), dtype=torch.float64, device="cuda")
    v = torch.empty((E,), dtype=torch.uint8, device="cuda")
    tf = torch.empty((E,), dtype=torch.float64, device="cuda")
    stt = torch.empty((E,), dtype=torch.int32, device="cuda")

    def call(E=E, maxd=1.0, mode=0, thr=0.0, it=64, slack=1e-6, valid=v.data_ptr(), t_free=tf.data_ptr(), status=stt.data_ptr(), h=dev._h):
        return lib.nbk_edge_continuous_batch(h, s.data_ptr(), g.data_ptr(), None, E, maxd, mode, thr, it, slack, valid, None,
                                             t_free, status, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert (stt.cpu().numpy() != DEGENERATE).all()
    nan = float("nan")
    for kw in (dict(it=0), dict(slack=-1.0), dict(slack=nan), dict(thr=nan), dict(maxd=nan), dict(maxd=0.0), dict(mode=2),
               dict(E=-1), dict(valid=None), dict(t_free=None), dict(status=None), dict(h=None)):
        assert call(**kw) == -1, kw
    assert call(E=0, valid=None) == 0
    with pytest.raises(_lib.NbkError):
        dev.edge_continuous(s, g, 1.0, max_iter=0)
