"""NumPy + CPU-oracle restatement of nbk_spline_cloud_continuous_batch (DeviceModel.cloud_spline_continuous,
ContinuousConnector.validate_trajectories(..., cloud=...)), for the tests.

One item per (trajectory, selected robot shape).  The advance across the knot spans is the loop of
spline_continuous_ref.reference_spline_continuous (plain Python floats, every operation separately rounded), with mu per span from
nbk_spline_shape_motion_bounds_host; the distance is the three-way rule of cloud_continuous_ref.CloudDistance, written out again here
because that class computes its q(t) and its D_end from an edge's end points: q(t) from ``spline_ref.de_boor``, the cut at D_end =
(thr + slack) + mu_max (1 - t) with mu_max the largest span bound of the item.  The per-trajectory reduction is
``ca_ref.reduce_items``; the accumulate form reduces over the scene's items and the cloud's together.

mu comes from the library's own host routine, as the other restatements take theirs: what the device is held against here is the
loop and the distance rule.  That the routine computes the right bounds is tests/test_cloud_spline_host.py's business (an independent
NumPy construction from the model arrays, and the pair bound of the same shape against a world shape).

``per_span_cut=True`` is the UNSOUND variant the header warns about (D_end from the current span's mu): the tests use it to show that
their fast-last-span trajectory is one it would free."""
import numpy as np

from numbotics_amd.engine import spline_shape_motion_bounds
from ca_ref import reduce_items, FREE, COLLISION, UNDECIDED
from cloud_cases import cloud_model
from cloud_continuous_ref import selection, EXIT_POINT, EXIT_INF, EXIT_CAP, EXIT_NAN
from continuous_ref import pair_distances
from spline_ref import de_boor
from spline_continuous_ref import degenerate, span_of, reference_spline_continuous


class CloudSplineDistance:
    """d of the items (trajectory, k-th selected shape) at t, by the rule of the header; counts the exits it takes (``exits``, indexed
    by cloud_continuous_ref's EXIT_*)."""

    def __init__(self, sm, pts, r, shapes, ctrl, knots, k, threshold, slack, look_ahead, per_span_cut=False):
        from oracle.cpu_oracle import Oracle
        self.sel = selection(sm, shapes)
        self.pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        self.orc = [Oracle(cloud_model(sm, self.pts, r, [int(x)])) for x in self.sel] if self.pts.shape[0] else []
        self.ctrl, self.knots, self.k = ctrl, knots, k
        self.mu = spline_shape_motion_bounds(sm, ctrl, knots, k)[:, :, self.sel]             # (S, spans, K); empty spans hold 0
        self.mu_max = self.mu.max(axis=1)                                                    # (S, K)
        self.per_span_cut = per_span_cut
        self.base = threshold + slack
        self.d_cap = self.base + look_ahead
        self.exits = np.zeros(4, dtype=np.int64)

    def __call__(self, ss, kk, tt):
        q = de_boor(self.ctrl, self.knots, self.k, ss, tt)
        fin = np.isfinite(q).all(axis=1)
        if self.per_span_cut:
            n = self.ctrl.shape[1]
            m = self.mu[ss, np.array([span_of(self.knots, n, self.k, t) - self.k for t in tt], dtype=np.int64), kk]
        else:
            m = self.mu_max[ss, kk]
        d_end = self.base + m * (1.0 - tt)
        D = np.where(d_end < self.d_cap, d_end, self.d_cap)
        d = np.full(ss.shape, np.nan)
        how = np.full(ss.shape, EXIT_NAN)
        for k in np.unique(kk):
            rows = np.nonzero((kk == k) & fin)[0]
            if rows.shape[0] == 0:
                continue
            dmin = pair_distances(self.orc[k], q[rows]).min(axis=1)
            near = dmin < D[rows]
            at_end = D[rows] == d_end[rows]
            d[rows] = np.where(near, dmin, np.where(at_end, np.inf, self.d_cap))
            how[rows] = np.where(near, EXIT_POINT, np.where(at_end, EXIT_INF, EXIT_CAP))
        self.exits += np.bincount(how, minlength=4)
        return d


def advance_span_items(distance, mu, knots, n, k, live, threshold, max_iter, slack):
    """The loop of include/nbk.h on items (S, K) across the knot spans (mu (S, spans, K)) -> stop (S, K), status (S, K)."""
    S, _, K = mu.shape
    kn = [float(x) for x in knots]
    t = np.zeros((S, K))
    ell = np.full((S, K), span_of(knots, n, k, 0.0))
    stop = np.full((S, K), np.nan)
    st = np.full((S, K), -1, dtype=np.int32)
    active = np.zeros((S, K), dtype=bool)
    active[live, :] = True
    for _ in range(max_iter):
        ss, pp = np.nonzero(active)
        if ss.shape[0] == 0:
            break
        d = distance(ss, pp, t[ss, pp])
        for s, p, dd in zip(ss, pp, d):
            tt, e = float(t[s, p]), int(ell[s, p])
            dd = float(dd)
            if dd <= threshold:
                stop[s, p], st[s, p], active[s, p] = tt, COLLISION, False
                continue
            gap = (dd - threshold) - slack
            if not gap > 0.0:
                stop[s, p], st[s, p], active[s, p] = tt, UNDECIDED, False
                continue
            m = float(mu[s, e - k, p])
            while True:
                hi = kn[e + 1]
                if m == 0.0:
                    tt = hi
                else:
                    tn = tt + gap / m
                    if not tn >= hi:
                        tt = tn
                        break
                    used = m * (hi - tt)
                    gap = gap - used
                    tt = hi
                if tt >= 1.0:
                    tt = 1.0
                    stop[s, p], st[s, p], active[s, p] = 1.0, FREE, False
                    break
                e = span_of(knots, n, k, tt)
                m = float(mu[s, e - k, p])
                if not gap > 0.0:
                    break
            t[s, p], ell[s, p] = tt, e
    ss, pp = np.nonzero(active)
    stop[ss, pp] = t[ss, pp]
    st[ss, pp] = UNDECIDED
    return stop, st


def reference_cloud_spline_continuous(sm, pts, r, ctrl, knots, k, threshold=0.0, max_iter=64, slack=1e-6, look_ahead=np.inf,
                                      shapes=None, scene_orc=None, per_span_cut=False):
    """-> valid (S,) bool, t_free (S,), status (S,) int32, the cloud items' stop points and statuses (S, K), and the count of distance
    evaluations by exit (EXIT_*).  ``scene_orc`` (the Oracle of ``sm``): the accumulate form -- the reduction runs over the scene's
    (trajectory, pair) items and the cloud's together."""
    ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
    knots = np.asarray(knots, dtype=np.float64)
    S, n, _ = ctrl.shape
    deg = degenerate(ctrl, knots, k)
    K = selection(sm, shapes).shape[0]
    N = np.asarray(pts).reshape(-1, 3).shape[0]
    exits = np.zeros(4, dtype=np.int64)
    if K == 0 or N == 0 or deg.all():                    # nothing to hit, or nothing that runs: no items
        stop, st = np.zeros((S, 0)), np.zeros((S, 0), dtype=np.int32)
    else:
        safe = np.where(deg[:, None, None], 0.0, ctrl)   # (the items of degenerate trajectories never run; their bounds are not read)
        dist_fn = CloudSplineDistance(sm, pts, r, shapes, safe, knots, k, threshold, slack, look_ahead, per_span_cut)
        stop, st = advance_span_items(dist_fn, dist_fn.mu, knots, n, k, ~deg, threshold, max_iter, slack)
        exits = dist_fn.exits
    all_stop, all_st = stop, st
    if scene_orc is not None:
        ref = reference_spline_continuous(sm, scene_orc, ctrl, knots, k, threshold=threshold, max_iter=max_iter, slack=slack)
        all_stop, all_st = np.concatenate((ref[3], stop), axis=1), np.concatenate((ref[4], st), axis=1)
    valid, t_free, status = reduce_items(all_stop, all_st, np.ones(S), ~deg)
    return valid, t_free, status, stop, st, exits


def dense_cloud_spline_min_distance(sm, pts, r, shapes, ctrl, knots, k, n=2000):
    """min over n + 1 samples t in [0, 1], the selected shapes and the points of the signed distance on one spline ctrl (n_ctrl, nq)."""
    from oracle.cpu_oracle import Oracle
    t = np.linspace(0.0, 1.0, n + 1)
    q = de_boor(ctrl[None], knots, k, np.zeros(t.shape[0], dtype=np.int64), t)
    return min(pair_distances(Oracle(cloud_model(sm, pts, r, [int(x)])), q).min() for x in selection(sm, shapes))
