"""NumPy + CPU-oracle restatement of nbk_spline_continuous_batch (ContinuousConnector.validate_trajectories), for the tests.

Conservative advancement per (trajectory, pair) item across the knot spans: q(t) from ``spline_ref.de_boor`` (the bits of
``UnitBSpline.__call__``), distances from ``Oracle.pair_distances``, mu per span from ``spline_motion_bounds``, the loop of
include/nbk.h.  The advance runs per item in plain Python floats (every operation separately rounded, as the device's); the
per-trajectory reduction is ``ca_ref.reduce_items``."""
import math

import numpy as np

from numbotics_amd.engine import spline_motion_bounds
from ca_ref import reduce_items, FREE, COLLISION, UNDECIDED
from continuous_ref import pair_distances
from spline_ref import de_boor, speed_bound, MIN_SPEED, DBL_MAX


def knots_ok(knots, n, k):
    t = np.asarray(knots, dtype=np.float64)
    return bool(t.shape == (n + k + 1,) and np.isfinite(t).all() and (np.diff(t) >= 0.0).all()
                and (t[:k + 1] == 0.0).all() and (t[n:] == 1.0).all())


def degenerate(ctrl, knots, k):
    """(S,) bool: the trajectories nbk_spline_continuous_batch reports DEGENERATE."""
    S, n, _ = ctrl.shape
    if not knots_ok(knots, n, k):
        return np.ones(S, dtype=bool)
    out = np.zeros(S, dtype=bool)
    for s in range(S):
        V = speed_bound(ctrl[s], knots, k)
        out[s] = not np.isfinite(ctrl[s]).all() or not (V > MIN_SPEED and V <= DBL_MAX)
    return out


def span_of(knots, n, k, t):
    return min(max(int(np.searchsorted(knots, t, side="right")) - 1, k), n - 1)


def reference_spline_continuous(sm, orc, ctrl, knots, k, threshold=0.0, max_iter=64, slack=1e-6):
    """-> valid (S,) bool, t_free (S,), status (S,) int32, and the per-item stop points / statuses (S, P)."""
    ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
    knots = np.asarray(knots, dtype=np.float64)
    S, n, nq = ctrl.shape
    P = sm.n_pairs
    deg = degenerate(ctrl, knots, k)
    mu = spline_motion_bounds(sm, ctrl, knots, k) if (P > 0 and not deg.all()) else np.zeros((S, n - k, P))
    kn = [float(x) for x in knots]
    t = np.zeros((S, P))
    ell = np.full((S, P), span_of(knots, n, k, 0.0))
    stop = np.full((S, P), np.nan)
    st = np.full((S, P), -1, dtype=np.int32)
    active = np.zeros((S, P), dtype=bool)
    active[~deg, :] = True
    for _ in range(max_iter):
        ss, pp = np.nonzero(active)
        if ss.shape[0] == 0:
            break
        q = de_boor(ctrl, knots, k, ss, t[ss, pp])
        d = pair_distances(orc, q)[np.arange(ss.shape[0]), pp]
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
    return reduce_items(stop, st, np.ones(S), ~deg) + (stop, st)


def motion_bounds_numpy(sm, ctrl, knots, k):
    """mu (S, n - k, P) built independently from the model arrays (float64 NumPy, its own summation order): per non-empty span,
    the per-joint speed V and travel A of the control polygon, then the sum over the joints of either shape's own path."""
    kin = sm.kin
    J = kin.n_joints
    parent = np.asarray(kin.joint_parent)
    jtype = np.asarray(kin.joint_type)
    qidx = np.asarray(kin.joint_qidx)
    trans = np.asarray(kin.joint_trans, dtype=np.float64).reshape(J, 3)
    slide = np.asarray(kin.joint_slide, dtype=np.float64).reshape(J, 3)
    bound = _shape_bounds(sm)

    def path(f):
        out = []
        while f >= 0:
            out.append(int(f))
            f = parent[f]
        return out[::-1]

    ctrl = np.asarray(ctrl, dtype=np.float64)
    knots = np.asarray(knots, dtype=np.float64)
    S, n, _ = ctrl.shape
    R = sm.n_rshapes
    mu = np.zeros((S, n - k, sm.n_pairs))
    for ell in range(k, n):
        if not knots[ell] < knots[ell + 1]:
            continue
        den = np.array([knots[i + k + 1] - knots[i + 1] for i in range(ell - k, ell)])
        V = (k * np.abs(np.diff(ctrl[:, ell - k:ell + 1], axis=1)) / den[None, :, None]).max(axis=1)     # (S, nq)
        A = np.abs(ctrl[:, ell - k:ell + 1]).max(axis=1)                                                    # (S, nq)
        for p in range(sm.n_pairs):
            a, b = int(sm.pair_a[p]), int(sm.pair_b[p])
            pa = path(int(sm.rshape_frame[a]))
            pb = path(int(sm.rshape_frame[b])) if b < R else []
            total = np.zeros(S)
            for x, own, other in ((a, pa, pb), (b, pb, pa)):
                for i, j in enumerate(own):
                    if j in other:
                        continue
                    if jtype[j] == 1:
                        c = np.full(S, np.linalg.norm(slide[j]))
                    else:
                        below = own[i + 1:]
                        c = np.full(S, sum(np.linalg.norm(trans[q]) for q in below) + bound[x])
                        for q in below:
                            if jtype[q] == 1:
                                c = c + np.linalg.norm(slide[q]) * A[:, qidx[q]]
                    total = total + c * V[:, qidx[j]]
            mu[:, ell - k, p] = total
    return mu


def _shape_bounds(sm):
    """|local translation| + rho + margin of every robot shape (rho: the core's bounding radius)."""
    out = np.empty(sm.n_rshapes)
    for x in range(sm.n_rshapes):
        L = np.asarray(sm.rshape_local[x], dtype=np.float64).reshape(-1)
        typ, prm = int(sm.rshape_type[x]), np.asarray(sm.rshape_param[x], dtype=np.float64)
        margin = prm[3]
        if typ == 0:
            rho, margin = 0.0, prm[0]
        elif typ == 1:
            rho, margin = prm[1], prm[0]
        elif typ == 2:
            rho = np.linalg.norm(prm[:3] - margin)
        elif typ == 3:
            rho = math.hypot(prm[0] - margin, prm[1] - margin)
        else:
            h = int(prm[0])
            v = np.asarray(sm.hull_verts, dtype=np.float64).reshape(-1, 3)[sm.hull_vert_begin[h]:sm.hull_vert_begin[h + 1]]
            rho = np.linalg.norm(v, axis=1).max()
        out[x] = np.linalg.norm(L[[3, 7, 11]]) + rho + margin
    return out


def spline_from_edges(s, g, n=4, k=3):
    """Splines of degree k whose n control points lie evenly on the segments s -> g: each traces its segment (the clamped
    uniform spline of collinear, evenly spaced control points stays on the segment)."""
    w = np.linspace(0.0, 1.0, n)
    return (1.0 - w)[None, :, None] * s[:, None, :] + w[None, :, None] * g[:, None, :]


def dense_min_distance(orc, ctrl, knots, k, n=2000):
    """min over n + 1 samples t in [0, 1] and over the pairs of the signed distance on one spline ctrl (n_ctrl, nq)."""
    t = np.linspace(0.0, 1.0, n + 1)
    q = de_boor(ctrl[None], knots, k, np.zeros(t.shape[0], dtype=np.int64), t)
    return pair_distances(orc, q).min()
