"""The composition of tests/ca_key_cases.py, asserted on the restatements alone (no device): what tests/test_gpu_ca_keys.py places
side by side must be in the batches, whatever becomes of the scene or of the random edges."""
import numpy as np
import pytest

from oracle.cpu_oracle import Oracle
from numbotics_amd.planning import unit_knots
import ca_key_cases as K
from ca_ref import FREE, COLLISION, UNDECIDED, DEGENERATE
from continuous_ref import reference_continuous
from spline_continuous_ref import reference_spline_continuous
from cloud_continuous_ref import reference_cloud_continuous


def _counts(status):
    return {c: int((status == c).sum()) for c in (FREE, COLLISION, UNDECIDED, DEGENERATE)}


@pytest.mark.parametrize("max_iter", K.MAX_ITERS)
def test_edges_hold_every_status_and_a_collision_at_zero(fresh_world, max_iter):
    arm, chain, obs = K.scene()
    sm = arm.scene_model()
    s, g = K.edges(chain)
    assert s.shape[0] == 66 and K.tiled(s).shape[0] == 264
    valid, end, t_free, status, _, _ = reference_continuous(sm, Oracle(sm), s, g, K.MAX_DISTANCE["connect"], max_iter=max_iter)
    n = _counts(status)
    print(max_iter, n)
    assert n[DEGENERATE] == 2 and (status[-2:] == DEGENERATE).all()
    assert n[COLLISION] > 0 and n[UNDECIDED] > 0 and (n[FREE] > 0 or max_iter == 1), n
    at_zero = (status == COLLISION) & (t_free.view(np.int64) == np.float64(0.0).view(np.int64))
    assert at_zero.any(), "no edge collides at t = +0.0: no key is 0"
    assert (status[:K.N_KEPT] != DEGENERATE).all()


def test_splines_hold_the_three_degenerate_kinds(fresh_world):
    arm, chain, obs = K.scene()
    sm = arm.scene_model()
    c = K.splines(chain)
    assert c.shape == (67, 4, chain.dof) and K.tiled(c).shape[0] > 256
    valid, t_free, status, _, _ = reference_spline_continuous(sm, Oracle(sm), c, unit_knots(4, 3), 3)
    n = _counts(status)
    print(n)
    assert (status[-3:] == DEGENERATE).all() and n[DEGENERATE] == 3
    assert n[FREE] > 0 and n[COLLISION] > 0
    assert ((status == COLLISION) & (t_free.view(np.int64) == 0)).any()
    valid, t_free, status, _, _ = reference_spline_continuous(sm, Oracle(sm), c, K.unclamped_knots(), 3)
    assert (status == DEGENERATE).all() and np.isnan(t_free).all() and not valid.any()


def test_the_cloud_lowers_keys_the_scene_left(fresh_world):
    arm, chain, obs = K.scene()
    sm = arm.scene_model()
    orc = Oracle(sm)
    s, g = K.edges(chain)
    pts, shapes = K.cloud(sm)
    assert pts.shape[0] <= 64 and len(shapes) <= 3
    own = reference_continuous(sm, orc, s, g, K.MAX_DISTANCE["connect"])
    both = reference_cloud_continuous(sm, pts, K.CLOUD_R, s, g, K.MAX_DISTANCE["connect"], look_ahead=K.CLOUD_LOOK_AHEAD, shapes=shapes,
                                      scene_orc=orc)
    live = own[3] != DEGENERATE
    lowered = live & (both[2] < own[2])
    print(_counts(own[3]), _counts(both[3]), int(lowered.sum()))
    assert lowered.sum() >= 3, "the cloud stops no edge ahead of the scene"
    assert (live & (both[2] == own[2]) & (both[3] == own[3])).sum() >= 3, "the cloud stops every edge ahead of the scene"
    assert (both[3] == FREE).any() and (both[3][-2:] == DEGENERATE).all()
