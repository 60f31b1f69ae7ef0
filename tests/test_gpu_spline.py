"""B-spline trajectory checks on the device (nbk_spline_validity_batch: k_spline_plan, k_scan, k_spline_expand + the validity
pipeline per tile, k_spline_reduce): valid / n_samples equal and t_hit bit-identical to the NumPy + oracle restatement
(tests/spline_ref.py); the linear two-point spline equals the edge batch; tiling, a robot beyond the LDS-parked layout, a
descriptor without pairs, degenerate inputs, the connector API and the C layer's error codes.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd.planning import unit_bspline, unit_knots
from numbotics_amd.scenes import build_scene, sample_q
from test_gpu_parity import torch_cuda      # noqa: F401  (fixture)
from spline_ref import random_splines, reference_splines

SCENES = [("c2", True), ("c2", False), ("c3", True), ("c3", False), ("c2m", True), ("c2m", False)]
IDS = [f"{s}-{'bullet' if m else 'sharp'}" for s, m in SCENES]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_same(got, ref, what):
    v, th, ns = got
    rv, rth, rns = ref
    assert np.array_equal(ns, rns), f"{what}: n_samples differs on {np.nonzero(ns != rns)[0][:10]}"
    assert np.array_equal(v, rv), f"{what}: valid differs on {np.nonzero(v != rv)[0][:10]}"
    assert np.array_equal(_bits(th), _bits(rth)), f"{what}: t_hit differs on {np.nonzero(_bits(th) != _bits(rth))[0][:10]}"


def _free_q(orc, chain, seed):
    q = random_splines(chain, 2000, 2, seed)[:, 0] * 0.3
    return q[~orc.validity(q)][0]


@pytest.mark.parametrize("scene,margins", [("c2", True), ("c2", False), ("c3", True), ("c3", False)],
                         ids=["c2-bullet", "c2-sharp", "c3-bullet", "c3-sharp"])
def test_linear_spline_is_the_edge_batch(fresh_world, scene, margins, torch_cuda):
    arm, chain, obs = build_scene(scene, bullet_margins=margins)
    _, dev = arm._scene_device()
    rng = np.random.default_rng(21)
    E = 2400
    s = sample_q(chain, E, seed=22)
    g = sample_q(chain, E, seed=23)
    d = np.linalg.norm(g - s, axis=1)
    g = s + (g - s) * np.minimum(1.0, rng.uniform(0.05, 1.0, E) * np.pi / d)[:, None]
    g[:40] = s[:40]                                                   # degenerate: zero length
    g[40:80] = s[40:80] + 1e-9                                        # degenerate: below float32 eps
    for res in (0.05, 0.01):
        ok, _, ns = dev.edge_validity(s, g, res, np.pi, "connect")
        v, th, sns = dev.spline_validity(np.stack((s, g), axis=1), unit_knots(2, 1), 1, res)
        assert np.array_equal(sns, ns) and np.array_equal(v, ok), res
        assert (sns[:80] == 0).all() and not v[:80].any() and np.isnan(th[v]).all() and not np.isnan(th[~v & (sns > 0)]).any()
        assert 0 < v.sum() < E


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("scene,margins", SCENES, ids=IDS)
def test_bit_parity_with_the_restatement(fresh_world, scene, margins, k, torch_cuda):
    arm, chain, obs = build_scene(scene, bullet_margins=margins)
    sm = arm.scene_model()
    orc = Oracle(sm)
    _, dev = arm._scene_device()
    free = _free_q(orc, chain, 5)
    n_valid = n_hit = 0
    for i, n in enumerate(sorted({max(2, k + 1), (k + 13) // 2, 12})):
        c = random_splines(chain, 170, n, 1000 * k + n, near=free, spread=0.3)
        thr = (0.0, 0.01, -0.002)[i % 3]
        got = dev.spline_validity(c, unit_knots(n, k), k, 0.05, threshold=thr)
        ref = reference_splines(orc, c, unit_knots(n, k), k, 0.05, threshold=thr)
        _assert_same(got, ref, f"{scene} k={k} n={n} thr={thr}")
        n_valid += int(got[0].sum())
        n_hit += int((~got[0]).sum())
    assert n_valid > 0 and n_hit > 0


def test_batches_of_several_tiles(fresh_world, torch_cuda):
    arm, chain, obs = build_scene("c2")
    orc = Oracle(arm.scene_model())
    _, dev = arm._scene_device()
    free = _free_q(orc, chain, 7)
    c = random_splines(chain, 4000, 8, 77, near=free, spread=0.8)
    c[:2000] = free + (c[:2000] - free) * 0.12                       # the joint-box half, shrunk to a few hundred samples each
    got = dev.spline_validity(c, unit_knots(8, 3), 3, 0.01)
    assert int(got[2].sum()) > 2 * (1 << 20)
    _assert_same(got, reference_splines(orc, c, unit_knots(8, 3), 3, 0.01), "tiles")
    assert 0 < got[0].sum() < 4000


def test_robot_beyond_the_parked_layout(fresh_world, torch_cuda, tmp_path):
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
    c = random_splines(chain, 200, 6, 9, near=np.zeros(chain.dof), spread=0.15)
    for k in (1, 3):
        _assert_same(dev.spline_validity(c, unit_knots(6, k), k, 0.05), reference_splines(orc, c, unit_knots(6, k), k, 0.05),
                     f"big robot k={k}")
    # the same robot without any pair: only non-finite samples collide
    sm0 = arm.scene_model(pairs=[])
    assert sm0.n_pairs == 0
    dev0 = DeviceModel(sm0)
    c0 = c[:50].copy()
    c0[3, 2, 4] = np.inf                                                # a leg of infinite length: degenerate
    v, th, ns = dev0.spline_validity(c0, unit_knots(6, 5), 5, 0.05)
    _assert_same((v, th, ns), reference_splines(Oracle(sm0), c0, unit_knots(6, 5), 5, 0.05), "no pairs")
    assert ns[3] == 0 and v.sum() == 49
    c1, kn = _nan_at_the_end(c[:20, :3])
    v, th, ns = dev0.spline_validity(c1, kn, 1, 0.05)
    _assert_same((v, th, ns), reference_splines(Oracle(sm0), c1, kn, 1, 0.05), "no pairs, NaN sample")
    assert ns[9] > 0 and not v[9] and th[9] == 1.0 and v.sum() == 19


def _nan_at_the_end(c):
    """Knots [0, 0, 1, 1, 1]: the last leg has no span (den = 0, skipped by the speed bound), so a NaN in the last control point of
    trajectory 9 leaves V finite and reaches only the sample t = 1 (alpha = 0, 0 * NaN): a non-finite sample, which collides."""
    c = c.copy()
    c[9, 2] = np.nan
    return c, np.array([0.0, 0.0, 1.0, 1.0, 1.0])


def test_degenerate_trajectories(fresh_world, torch_cuda):
    arm, chain, obs = build_scene("c3")
    orc = Oracle(arm.scene_model())
    _, dev = arm._scene_device()
    free = _free_q(orc, chain, 3)
    c = random_splines(chain, 8, 5, 4, near=free, spread=0.05)
    c[1, 3, 2] = np.nan
    c[2] = free
    c[5, 0] = np.nan                                                    # NaN in the first control point
    v, th, ns = dev.spline_validity(c, unit_knots(5, 3), 3, 0.02)
    for s in (1, 2, 5):
        assert ns[s] == 0 and not v[s] and np.isnan(th[s])
    _assert_same((v, th, ns), reference_splines(orc, c, unit_knots(5, 3), 3, 0.02), "degenerate")
    assert (ns[[0, 3, 4, 6, 7]] > 0).all()
    c1, kn = _nan_at_the_end(random_splines(chain, 12, 3, 6, near=free, spread=0.05))
    v, th, ns = dev.spline_validity(c1, kn, 1, 0.02)
    _assert_same((v, th, ns), reference_splines(orc, c1, kn, 1, 0.02), "NaN sample")
    assert ns[9] > 0 and not v[9] and th[9] == 1.0


def test_connector_api(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd.planning.sampling_based import ConnectorParams, DiscreteConnector, EuclideanSpace, PlannerParams, PRM
    arm, chain, obs = build_scene("c3")
    orc = Oracle(arm.scene_model())
    lim = np.asarray(chain.joint_limits, dtype=np.float64)
    lim = np.where(np.isfinite(lim), lim, np.sign(lim) * np.pi)
    conn = DiscreteConnector(ConnectorParams(resolution=0.02, max_distance=1.0, arm=arm))
    prm = PRM(EuclideanSpace(lim[:, 0], lim[:, 1]), conn, PlannerParams(max_iters=600, k_nearest=10, goal_bias=0.05))
    q = sample_q(chain, 4000, seed=31) * 0.6
    goal = q[~orc.validity(q) & (np.linalg.norm(q, axis=1) > 2.5)][0]
    prm.add_start(np.zeros(chain.dof))
    prm.add_goal(goal)
    rng = np.random.default_rng(3)
    prm.plan([goal.copy() if rng.random() < 0.05 else rng.uniform(lim[:, 0], lim[:, 1]) for _ in range(600)])
    sol = prm.solution()
    assert sol is not None
    path = np.stack([nd.state for nd in sol])
    assert path.shape[0] >= 3
    k = min(3, path.shape[0] - 1)
    spl = unit_bspline(path, degree=k)
    ok, t_hit = conn.validate_trajectory(spl)
    rv, rth, rns = reference_splines(orc, path[None], spl.t, k, 0.02)
    assert ok == bool(rv[0]) and _bits([t_hit])[0] == _bits(rth)[0]
    # batches: NumPy in / NumPy out, device tensors stay on the device
    free = _free_q(orc, chain, 11)
    c = random_splines(chain, 64, 7, 12, near=free, spread=0.4)
    a = conn.validate_trajectories(c, degree=4)
    tc = torch.from_numpy(c).cuda()
    b = conn.validate_trajectories(tc, degree=4)
    assert all(torch.is_tensor(x) and x.is_cuda for x in b)
    _assert_same(a, tuple(x.cpu().numpy() for x in b), "numpy vs tensor")
    _assert_same(a, reference_splines(orc, c, unit_knots(7, 4), 4, 0.02), "connector")
    assert isinstance(a[0], np.ndarray) and a[0].dtype == bool and a[2].dtype == np.int32


def test_error_codes_and_capture(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd import _lib
    arm, chain, obs = build_scene("c2")
    _, dev = arm._scene_device()
    lib = _lib.load()
    S, n, k, nq = 4, 6, 3, chain.dof
    ctrl = torch.from_numpy(random_splines(chain, S, n, 2) * 0.2).cuda()
    v = torch.zeros((S,), dtype=torch.uint8, device="cuda")
    th = torch.zeros((S,), dtype=torch.float64, device="cuda")
    ns = torch.zeros((S,), dtype=torch.int32, device="cuda")
    kn0 = unit_knots(n, k)

    def call(S=S, n=n, k=k, knots=kn0, res=0.05, thr=0.0, ctrl_p=ctrl.data_ptr(), valid=v.data_ptr(), h=dev._h, st=None):
        kp = None if knots is None else np.ascontiguousarray(knots, dtype=np.float64)
        return lib.nbk_spline_validity_batch(h, ctrl_p, S, n, k, None if kp is None else kp.ctypes.data, res, thr, valid,
                                             th.data_ptr(), ns.data_ptr(), st)
    assert call() == 0
    torch.cuda.synchronize()
    ref = [x.clone() for x in (v, th, ns)]
    assert (ns.cpu().numpy() > 0).all()
    nan, inf = float("nan"), float("inf")
    bad = [dict(k=0), dict(k=6, n=8, knots=unit_knots(8, 6)), dict(n=3, knots=unit_knots(3, 3)), dict(n=70000, knots=unit_knots(70000, 3)),
           dict(knots=kn0 * 2.0), dict(knots=kn0 - 0.25), dict(knots=np.where(kn0 == 1.0, nan, kn0)),
           dict(knots=np.concatenate((kn0[:5], [0.2], kn0[6:]))), dict(res=0.0), dict(res=-1.0), dict(res=nan), dict(res=inf),
           dict(S=-1), dict(ctrl_p=None), dict(valid=None), dict(h=None), dict(knots=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(S=0, ctrl_p=None, valid=None) == 0
    # inside a capture: refused before any synchronisation or allocation; the capture and the stream stay usable
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sst = C.c_void_p(side.cuda_stream)
        g0 = torch.cuda.CUDAGraph()
        g0.capture_begin()
        assert call(st=sst) == -4
        g0.capture_end()
        v.zero_(); th.zero_(); ns.zero_()
        assert call(st=sst) == 0
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip((v, th, ns), ref):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
    with pytest.raises(_lib.NbkError):
        dev.spline_validity(ctrl, kn0 * 2.0, k, 0.05)
