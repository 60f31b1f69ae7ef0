"""NumPy + CPU-oracle restatement of nbk_spline_cloud_validity_batch (DeviceModel.cloud_spline_validity,
DiscreteConnector.validate_trajectories(..., cloud=...)), for the tests.

The trajectory rule is tests/spline_ref.py's (``spline_samples``: V, the degenerate rule, the sample times, de Boor), the verdict of a
sample ``cloud_cases.cloud_mask``'s (the oracle on the descriptor that holds the points as sphere world shapes; a non-finite row
collides there too).  On top of them: the first colliding sample, the cloud's status, knots that break the rules, a trajectory of too
many samples, and the accumulate form (only the samples before the t_hit that comes in are looked at)."""
import numpy as np

from cloud_cases import cloud_mask
from spline_ref import spline_samples
from spline_continuous_ref import knots_ok


def reference_cloud_splines(sm, pts, r, ctrl, knots, k, resolution, threshold=0.0, shapes=None, status=0, prev=None):
    """-> valid (S,) bool, t_hit (S,), n_samples (S,) int32 of nbk_spline_cloud_validity_batch.  ``status``: the cloud's (2: a
    non-finite point came with its last update).  ``prev`` = (valid, t_hit) or (valid, None): the accumulate form, on what
    nbk_spline_validity_batch wrote for the same trajectories."""
    ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
    knots = np.asarray(knots, dtype=np.float64)
    S, n, _ = ctrl.shape
    valid = np.zeros(S, dtype=bool)
    t_hit = np.full(S, np.nan)
    ns = np.zeros(S, dtype=np.int32)
    if prev is not None:
        valid[:] = prev[0]
        if prev[1] is not None:
            t_hit[:] = prev[1]
    if not knots_ok(knots, n, k):
        return np.zeros(S, dtype=bool), np.full(S, np.nan), ns
    rows, owner, times = [], [], []
    for s in range(S):
        try:
            t, q = spline_samples(ctrl[s], knots, k, resolution)
        except ValueError:                               # more than 2^31 - 1 samples: none is looked at
            valid[s], t_hit[s], ns[s] = False, np.nan, -1
            continue
        ns[s] = t.shape[0]
        if t.shape[0] == 0:                              # degenerate
            valid[s], t_hit[s] = False, np.nan
            continue
        if status != 0:                                  # hit at the first sample, whatever came in
            valid[s], t_hit[s] = False, 0.0
            continue
        if prev is None:
            valid[s] = True
            look = np.ones(t.shape[0], dtype=bool)
        elif prev[0][s]:
            look = np.ones(t.shape[0], dtype=bool)
        elif prev[1] is None:
            continue                                     # stays 0, nothing is looked at
        else:
            look = t < prev[1][s]                        # (a NaN t_hit: nothing)
        rows.append(q[look])
        times.append(t[look])
        owner.append(np.full(int(look.sum()), s))
    if rows:
        q, t, owner = np.concatenate(rows), np.concatenate(times), np.concatenate(owner)
        hit = cloud_mask(sm, pts, r, q, threshold, shapes) if q.shape[0] else np.zeros(0, dtype=bool)
        hit = hit | ~np.isfinite(q).all(axis=1)          # (also where cloud_mask has no pair to ask: nbk_cloud_validity_batch's rule)
        for s in np.unique(owner[hit]):
            valid[s] = False
            t_hit[s] = t[hit & (owner == s)].min()       # the smallest colliding sample (below what came in, by `look`)
    return valid, t_hit, ns


def merge_scene_and_cloud(scene, cloud):
    """(valid, t_hit, n_samples) of the scene's call followed by the cloud's accumulating one, from the two separate references:
    invalid when either is, t_hit the smaller of the two."""
    valid = scene[0] & cloud[0]
    with np.errstate(invalid="ignore"):
        t_hit = np.fmin(scene[1], cloud[1])
    assert np.array_equal(scene[2], cloud[2])
    return valid, t_hit, scene[2]
