"""Proximity records and gradient rows of chosen (configuration, pair) items (nbk_pair_records_items, Arm.pair_proximity_jacobians /
item_proximity_jacobians / closest_proximity_jacobians): every field bit-identical to the matching entry of the all-pairs path
(k_distances<3>) and of the CPU oracle.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd.scenes import build_scene, sample_q
from test_gpu_parity import assert_bitwise, _tree_scene, torch_cuda      # noqa: F401  (fixture)

CYLINDER, HULL = 3, 5
SCENES = [("c2", True), ("c2", False), ("c3", True), ("tree", True), ("c2m", True), ("c5m", True), ("c5m", False)]


def _scene(name, margins):
    if name == "tree":
        return _tree_scene()
    return build_scene(name, bullet_margins=margins)


def _pair_kinds(sm):
    """(P,) bool: the pair has a cylinder or hull shape (exact depth through EPA); (P,) bool: robot-robot pair (shared joints)."""
    S = sm.n_rshapes
    ka = sm.rshape_type[sm.pair_a]
    robot_b = sm.pair_b < S
    kb = np.where(robot_b, sm.rshape_type[np.minimum(sm.pair_b, S - 1)], sm.wshape_type[np.maximum(sm.pair_b - S, 0)])
    epa = np.isin(ka, (CYLINDER, HULL)) | np.isin(kb, (CYLINDER, HULL))
    return epa, robot_b


@pytest.mark.parametrize("scene,margins", SCENES, ids=[f"{s}-{'bullet' if m else 'sharp'}" for s, m in SCENES])
def test_item_records_bitwise(fresh_world, scene, margins, torch_cuda):
    arm, chain, obs = _scene(scene, margins)
    sm = arm.scene_model()
    _, dev = arm._scene_device()
    P = sm.n_pairs
    B = 400 if scene in ("c2m", "c5m") else 1000
    q = sample_q(chain, B, seed=53)
    dr, wr, rr = Oracle(sm).proximity_jacobian(q)
    d_all, w_all, r_all = arm.proximity_jacobians(q)
    assert_bitwise(d_all, dr, "all-pairs distances vs oracle")
    epa, robot_pair = _pair_kinds(sm)
    rng = np.random.default_rng(7)
    # random items over every (b, p), with repeats, plus every overlapping cylinder / hull entry (the EPA replacement)
    deep = np.argwhere((dr < 0) & epa[None, :])
    if scene in ("c2", "c5m"):
        assert deep.shape[0] > 0, "no overlapping cylinder / hull items in the sample"
    assert robot_pair.any()
    for N in (1, 63, 64, 65, 20000):
        items = np.stack((rng.integers(0, B, N), rng.integers(0, P, N)), axis=1).astype(np.int32)
        if N == 20000:
            items = np.concatenate((items, deep.astype(np.int32), items[:100]))      # repeats
            rng.shuffle(items)
            sel_b, sel_p = items[:, 0], items[:, 1]
            if scene in ("c2", "c5m"):
                assert ((dr[sel_b, sel_p] < 0) & epa[sel_p]).any()
            assert robot_pair[sel_p].any(), "no robot-robot items (shapes sharing joints)"
        b, p = items[:, 0], items[:, 1]
        d, w, j = dev.pair_records(q, items)
        assert_bitwise(d, dr[b, p], f"{scene} N={N} distance")
        assert_bitwise(w, wr[b, p], f"{scene} N={N} witness")
        assert_bitwise(j, rr[b, p], f"{scene} N={N} rows")
        assert_bitwise(j, r_all[b, p], f"{scene} N={N} rows vs the all-pairs kernel")
        d1, w1, j1 = dev.pair_records(q, items, witness=False)
        assert w1 is None
        assert_bitwise(d1, d, "distance without witness")
        assert_bitwise(j1, j, "rows without witness")
        d2, w2, j2 = dev.pair_records(q, items, jacobian=False)
        assert j2 is None
        assert_bitwise(d2, d, "distance without rows")
        assert_bitwise(w2, w, "witness without rows")


@pytest.mark.parametrize("scene", ["c2", "c5m", "tree"])
def test_pair_subset_columns(fresh_world, scene, torch_cuda):
    """pair_proximity_jacobians(q, pairs) == proximity_jacobians(q)[:, pairs]: pair-major items, so waves are pair-uniform (the
    hull support's scalar-cache path); repeats and any order; CUDA tensor in, CUDA tensor out, same bits."""
    torch = torch_cuda
    arm, chain, obs = _scene(scene, True)
    P = arm.scene_model().n_pairs
    q = sample_q(chain, 3001, seed=59)
    d_all, w_all, r_all = arm.proximity_jacobians(q)
    rng = np.random.default_rng(3)
    for pairs in ([0], [P - 1, 0, P - 1, 1], list(rng.permutation(P)[:16]), list(range(P))):
        d, w, j = arm.pair_proximity_jacobians(q, pairs)
        assert d.shape == (3001, len(pairs)) and w.shape == (3001, len(pairs), 9) and j.shape == (3001, len(pairs), arm.dof)
        assert_bitwise(d, d_all[:, pairs], f"{scene} {pairs[:4]} distance")
        assert_bitwise(w, w_all[:, pairs], f"{scene} {pairs[:4]} witness")
        assert_bitwise(j, r_all[:, pairs], f"{scene} {pairs[:4]} rows")
    qt = torch.from_numpy(q).cuda()
    dt, wt, jt = arm.pair_proximity_jacobians(qt, np.array([2, 0, 2]))
    assert dt.is_cuda and wt.is_cuda and jt.is_cuda
    assert_bitwise(dt.cpu().numpy(), d_all[:, [2, 0, 2]], "tensor distance")
    assert_bitwise(jt.cpu().numpy(), r_all[:, [2, 0, 2]], "tensor rows")
    # one pair per configuration
    pair = rng.integers(0, P, 3001)
    d, w, j = arm.item_proximity_jacobians(q, pair)
    i = np.arange(3001)
    assert_bitwise(d, d_all[i, pair], "item distance")
    assert_bitwise(w, w_all[i, pair], "item witness")
    assert_bitwise(j, r_all[i, pair], "item rows")
    dt, _, jt = arm.item_proximity_jacobians(qt, torch.from_numpy(pair).cuda())
    assert jt.is_cuda and np.array_equal(jt.cpu().numpy(), j) and np.array_equal(dt.cpu().numpy(), d)


@pytest.mark.parametrize("scene", ["c2", "c5m"])
def test_closest_pair_records(fresh_world, scene, torch_cuda):
    torch = torch_cuda
    arm, chain, obs = _scene(scene, True)
    sm = arm.scene_model()
    B = 600
    q = sample_q(chain, B, seed=61)
    d_ref, i_ref = Oracle(sm).closest(q)
    d, pair, w, j = arm.closest_proximity_jacobians(q)
    assert pair.dtype == np.int32
    assert_bitwise(d, d_ref, "closest distance")
    assert np.array_equal(pair, i_ref), "argmin (first minimum)"
    d_all, w_all, r_all = arm.proximity_jacobians(q)
    i = np.arange(B)
    assert_bitwise(d_all[i, pair], d, "record distance at the argmin")
    assert_bitwise(w, w_all[i, pair], "witness at the argmin")
    assert_bitwise(j, r_all[i, pair], "rows at the argmin")
    for k in (0, 1, 7):
        prox = arm.closest_to(q[k])
        assert prox.distance == d[k]
        assert np.array_equal(prox.position_on_subject, w[k, 0:3]) and np.array_equal(prox.position_on_target, w[k, 3:6])
        assert np.array_equal(prox.normal_target_to_subject, w[k, 6:9])
        assert sm.pair_members(int(pair[k])) == (prox.subject, prox.target)
    dt, pt, wt, jt = arm.closest_proximity_jacobians(torch.from_numpy(q).cuda())
    assert jt.is_cuda and pt.dtype == torch.int32
    assert np.array_equal(pt.cpu().numpy(), pair) and np.array_equal(jt.cpu().numpy(), j) and np.array_equal(dt.cpu().numpy(), d)


def test_out_of_range_items_and_status_codes(fresh_world, torch_cuda):
    torch = torch_cuda
    from numbotics_amd import _lib
    arm, chain, obs = build_scene("c2")
    _, dev = arm._scene_device()
    P, B = arm.scene_model().n_pairs, 64
    big = torch.from_numpy(sample_q(chain, B + 16, seed=67)).cuda()
    q = big[8:8 + B]                       # rows -8..-1 and B..B+7 are valid memory: an unguarded kernel would read them silently
    items = np.array([[0, 0], [-1, 0], [B, 1], [3, -1], [3, P], [B - 1, P - 1], [-5, P + 2]], dtype=np.int32)
    d, w, j = dev.pair_records(q, torch.from_numpy(items).cuda())
    d, w, j = d.cpu().numpy(), w.cpu().numpy(), j.cpu().numpy()
    bad = np.array([False, True, True, True, True, False, True])
    assert np.isnan(d[bad]).all() and np.isnan(w[bad]).all() and np.isnan(j[bad]).all()
    d_all, w_all, r_all = arm.proximity_jacobians(q.cpu().numpy())
    assert_bitwise(d[~bad], d_all[[0, B - 1], [0, P - 1]], "in-range items beside out-of-range ones")
    assert_bitwise(j[~bad], r_all[[0, B - 1], [0, P - 1]], "in-range rows")
    # C status codes
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    it = torch.from_numpy(items).cuda()
    out = torch.empty((len(items),), dtype=torch.float64, device="cuda")
    f = lib.nbk_pair_records_items
    assert f(None, q.data_ptr(), B, it.data_ptr(), len(items), out.data_ptr(), None, None, st) == -1
    assert f(dev._h, q.data_ptr(), -1, it.data_ptr(), len(items), out.data_ptr(), None, None, st) == -1
    assert f(dev._h, q.data_ptr(), B, it.data_ptr(), -1, out.data_ptr(), None, None, st) == -1
    assert f(dev._h, None, B, it.data_ptr(), len(items), out.data_ptr(), None, None, st) == -1
    assert f(dev._h, q.data_ptr(), B, None, len(items), out.data_ptr(), None, None, st) == -1
    assert f(dev._h, q.data_ptr(), B, it.data_ptr(), len(items), None, None, None, st) == -1
    assert f(dev._h, None, B, None, 0, None, None, None, st) == 0                       # N == 0: nothing to launch
    assert f(dev._h, q.data_ptr(), B, it.data_ptr(), len(items), out.data_ptr(), None, None, st) == 0
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()[bad]).all()


def test_rerouted_scalar_and_iris_paths(fresh_world, torch_cuda):
    """distance_to / jacobian_proximity / distance_and_gradient now compute the selected pairs only: same records as the
    all-pairs path."""
    from numbotics_amd.planning.safe_sets import distance_and_gradient
    arm, chain, obs = build_scene("c5m")
    sm = arm.scene_model()
    q = sample_q(chain, 300, seed=71)
    dr, wr, rr = Oracle(sm).proximity_jacobian(q)
    target = obs[0]
    sel = arm._pair_selection(sm, target, None)
    prox = arm.distance_to(q[0], target)
    assert len(prox) == len(sel) >= 1
    for p, k in zip(prox, sel):
        assert p.distance == dr[0, k] and np.array_equal(p.position_on_subject, wr[0, k, 0:3])
    J = np.atleast_2d(arm.jacobian_proximity(q[0], target))
    assert_bitwise(J, rr[0, sel], "jacobian_proximity rows")
    link = prox[0].subject
    dist, grad = distance_and_gradient(arm, q, link, target)
    s = arm._pair_selection(sm, target, link)
    k = dr[:, s].argmin(axis=1)
    assert_bitwise(dist, dr[:, s].min(axis=1), "distance_and_gradient distance")
    assert_bitwise(grad, rr[:, s][np.arange(300), k], "distance_and_gradient rows")
