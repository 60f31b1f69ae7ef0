"""ContinuousConnector without a GPU: the motion bound mu (nbk_edge_motion_bounds_host), the NumPy + oracle restatement of the
certified loop (tests/continuous_ref.py), the thin-plate scene that discrete checks step over, and the host API."""
import numpy as np
import pytest

from oracle.cpu_oracle import Oracle
from numbotics_amd.scenes import build_scene
from continuous_ref import (dense_min_distance, motion_bounds_numpy, random_edges, random_scene, reference_continuous,
                            thin_plate_scene, tree_scene, FREE)

# |d(t) - d(t')| <= mu |t - t'| holds for the exact distances; the computed ones carry the narrowphase's own error (GJK's
# termination rule is relative), which reaches ~2e-6 m, 3e-6 relative, between two shapes on ONE rigid body of a random mechanism
# (mu = 0).  Checked here to the exact bound plus that relative allowance; DESIGN section 0 records what it means for the slack.
TOL_ABS, TOL_REL = 1e-9, 5e-6

SCENES = [("c2", True), ("c2", False), ("c3", True), ("c3", False), ("c2m", True), ("c2m", False), ("tree", True)]


def _scene(name, margins):
    if name == "tree":
        return tree_scene()
    return build_scene(name, bullet_margins=margins)


@pytest.mark.parametrize("scene,margins", SCENES + [("rand", s) for s in (3, 11, 29)])
def test_mu_is_a_lipschitz_bound(fresh_world, tmp_path, scene, margins):
    from numbotics_amd.engine import edge_motion_bounds
    if scene == "rand":
        built = random_scene(margins, tmp_path)
        if built is None:
            pytest.skip("random mechanism without joints or pairs")
        arm, chain, obs = built
    else:
        arm, chain, obs = _scene(scene, margins)
    sm = arm.scene_model()
    orc = Oracle(sm)
    s, g = random_edges(chain, 6, 17, scale=0.5)
    mu = edge_motion_bounds(sm, s, g)
    t = np.linspace(0.0, 1.0, 200)
    dt = np.abs(t[:, None] - t[None, :])
    checked = 0
    for e in range(s.shape[0]):
        q = (1.0 - t)[:, None] * s[e] + t[:, None] * g[e]
        d = orc.pair_distances(q)                                   # (200, P)
        for p in range(sm.n_pairs):
            pos = d[:, p] > 0.0
            both = pos[:, None] & pos[None, :]
            lhs = np.abs(d[:, p][:, None] - d[:, p][None, :])
            tol = TOL_ABS + TOL_REL * np.maximum(d[:, p][:, None], d[:, p][None, :])
            bad = both & (lhs > mu[e, p] * dt + tol)
            assert not bad.any(), f"edge {e} pair {p}: |d(t) - d(t')| exceeds mu |t - t'| (mu = {mu[e, p]})"
            checked += int(both.sum())
    assert checked > 0


@pytest.mark.parametrize("scene,margins", SCENES + [("rand", 3), ("rand", 11)])
def test_mu_matches_an_independent_numpy_construction(fresh_world, tmp_path, scene, margins):
    from numbotics_amd.engine import edge_motion_bounds
    if scene == "rand":
        built = random_scene(margins, tmp_path)
        if built is None:
            pytest.skip("random mechanism without joints or pairs")
        arm, chain, obs = built
    else:
        arm, chain, obs = _scene(scene, margins)
    sm = arm.scene_model()
    s, g = random_edges(chain, 12, 5)
    mu = edge_motion_bounds(sm, s, g)
    ref = motion_bounds_numpy(sm, s, g)
    assert mu.shape == (12, sm.n_pairs)
    np.testing.assert_allclose(mu, ref, rtol=1e-12, atol=0.0)
    assert (mu >= 0).all()


@pytest.mark.parametrize("scene,thr", [("c2", 0.0), ("c3", 0.01), ("tree", -0.002)])
def test_reference_loop_is_sound(fresh_world, scene, thr):
    arm, chain, obs = _scene(scene, True)
    sm = arm.scene_model()
    orc = Oracle(sm)
    s, g = random_edges(chain, 40, 23, scale=0.3)
    valid, end, t_free, status, _, _ = reference_continuous(sm, orc, s, g, 1.0, threshold=thr)
    assert valid.any() and (~valid).any()
    assert np.array_equal(valid, status == FREE)
    for e in np.nonzero(valid)[0]:
        assert dense_min_distance(orc, s[e], g[e]) > thr, f"edge {e} certified free but a dense sample is within the threshold"


def test_thin_plate_is_stepped_over_by_discrete_checks(fresh_world):
    from numbotics_amd.planning.sampling_based import ConnectorParams, DiscreteConnector
    arm, chain, obs = thin_plate_scene()
    sm = arm.scene_model()
    orc = Oracle(sm)
    s, g = random_edges(chain, 400, 5, scale=0.4)
    keep = ~orc.validity(s) & ~orc.validity(g)
    s, g = s[keep], g[keep]
    dv, _, _ = orc.edge_validity(s, g, 0.05, 10.0, "connect")
    hits = [e for e in np.nonzero(dv)[0] if dense_min_distance(orc, s[e], g[e]) <= 0.0]
    assert hits, "no edge crosses the plate between two discrete samples"
    e = hits[0]
    disc = DiscreteConnector(ConnectorParams(resolution=0.05, max_distance=10.0,
                                             validity_checker=lambda q: not orc.validity(q[None])[0]))
    assert disc.connect(s[e], g[e]) is not None                     # the discrete connector returns the goal
    valid, _, _, status, _, _ = reference_continuous(sm, orc, s[hits], g[hits], 10.0)
    assert not valid.any(), "the continuous check accepted an edge through the plate"


def test_host_api_checks_and_export():
    import numbotics_amd.planning.sampling_based as sb
    from numbotics_amd import _lib
    from numbotics_amd.planning.sampling_based import ConnectorParams, ContinuousConnector
    assert "ContinuousConnector" in sb.__all__
    for name in ("nbk_edge_continuous_batch", "nbk_edge_motion_bounds_host"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    params = ConnectorParams(validity_checker=lambda q: 1.0)
    with pytest.raises(ValueError):
        ContinuousConnector(params, max_iter=0)
    with pytest.raises(ValueError):
        ContinuousConnector(params, slack=-1e-9)
    with pytest.raises(ValueError):
        ContinuousConnector(params, slack=float("nan"))
    with pytest.raises(ValueError):
        ContinuousConnector(params).connect_batch(np.zeros((2, 3)), np.ones((2, 3)))     # no arm: no batched path


def test_motion_bounds_host_rejects_bad_descriptors(fresh_world):
    import ctypes as C
    from numbotics_amd import _lib
    from numbotics_amd.engine import model_desc
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    d, keep = model_desc(sm)
    lib = _lib.load()
    s = np.zeros((2, sm.kin.n_q))
    mu = np.empty((2, sm.n_pairs))
    assert lib.nbk_edge_motion_bounds_host(None, s.ctypes.data, s.ctypes.data, 2, mu.ctypes.data) == -1
    assert lib.nbk_edge_motion_bounds_host(C.byref(d), s.ctypes.data, s.ctypes.data, -1, mu.ctypes.data) == -1
    assert lib.nbk_edge_motion_bounds_host(C.byref(d), None, s.ctypes.data, 2, mu.ctypes.data) == -1
    pa = np.array(sm.pair_a, dtype=np.int32)
    pa[0] = sm.n_rshapes                                   # out of range
    d.pair_a = pa.ctypes.data
    assert lib.nbk_edge_motion_bounds_host(C.byref(d), s.ctypes.data, s.ctypes.data, 2, mu.ctypes.data) == -1
    assert mu.shape == (2, sm.n_pairs)


def test_scipy_path_on_an_analytic_checker():
    """1-D: the signed distance to a wall of width 2 mm at x = 0.5; the discrete connector at resolution 0.05 steps over it."""
    from numbotics_amd.planning.sampling_based import ConnectorParams, ContinuousConnector, DiscreteConnector
    wall = lambda q: abs(float(q[0]) - 0.5) - 0.001               # noqa: E731
    params = ConnectorParams(resolution=0.05, max_distance=10.0, validity_checker=wall)
    a, b, c = np.array([0.013]), np.array([1.013]), np.array([0.4])
    cc = ContinuousConnector(params)
    assert cc.is_valid(a) and not cc.is_valid(np.array([0.5]))
    disc = DiscreteConnector(ConnectorParams(resolution=0.05, max_distance=10.0, validity_checker=lambda q: wall(q) > 0.0))
    assert disc.connect(a, b) is not None                          # samples at 0.013 + 0.05 k miss the wall
    assert cc.connect(a, b) is None                                # crosses the wall
    assert np.array_equal(cc.connect(a, c), c)                     # stops short of it
    assert cc.connect(a, a) is None                                # degenerate
    short = ConnectorParams(resolution=0.05, max_distance=0.2, validity_checker=wall)
    end = ContinuousConnector(short).steer(a, b)                   # steering stops at max_distance, before the wall
    np.testing.assert_allclose(end, [0.213], rtol=1e-12)
