"""What the restatements of the certified entry points share (continuous_ref, spline_continuous_ref, cloud_continuous_ref): the
status codes, the conservative-advancement loop on items of ONE span, and the reduction of the items' stop points per trajectory."""
import numpy as np

FREE, COLLISION, UNDECIDED, DEGENERATE = 0, 1, 2, 3
RANK = {COLLISION: 0, UNDECIDED: 1, FREE: 2}


def advance_items(distance, mu, Tf, live, threshold, max_iter, slack):
    """The loop of include/nbk.h on items (E, K) of trajectories that are one span [0, Tf[e]], with ``distance(ee, kk, tt)`` the
    items' distances at tt -> stop (E, K), status (E, K) (NaN / -1 for the items of trajectories that are not ``live``).  The items
    of one iteration are evaluated together."""
    E, K = mu.shape
    t = np.zeros((E, K))
    stop = np.full((E, K), np.nan)
    st = np.full((E, K), -1, dtype=np.int32)
    active = np.zeros((E, K), dtype=bool)
    active[live, :] = True
    for _ in range(max_iter):
        ee, kk = np.nonzero(active)
        if ee.shape[0] == 0:
            break
        tt = t[ee, kk]
        d = distance(ee, kk, tt)
        m = mu[ee, kk]
        col = d <= threshold
        with np.errstate(invalid="ignore"):
            gap = (d - threshold) - slack
        und = ~col & ~(gap > 0.0)
        rest = ~col & ~und
        free0 = rest & (m == 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            tn = tt + gap / m
        free1 = rest & ~free0 & (tn >= Tf[ee])
        adv = rest & ~free0 & ~free1
        for mask, code in ((col, COLLISION), (und, UNDECIDED)):
            stop[ee[mask], kk[mask]] = tt[mask]
            st[ee[mask], kk[mask]] = code
        fr = free0 | free1
        stop[ee[fr], kk[fr]] = Tf[ee[fr]]
        st[ee[fr], kk[fr]] = FREE
        active[ee[~adv], kk[~adv]] = False
        t[ee[adv], kk[adv]] = tn[adv]
    ee, kk = np.nonzero(active)
    stop[ee, kk] = t[ee, kk]
    st[ee, kk] = UNDECIDED
    return stop, st


def reduce_items(stop, st, Tf, live):
    """Per trajectory the smallest stop point over its items, COLLISION before UNDECIDED before FREE on a tie, from "FREE at Tf"
    (explicit loops) -> valid (E,) bool, t_free (E,), status (E,) int32; 0 / NaN / DEGENERATE where not ``live``."""
    E = stop.shape[0]
    valid = np.zeros(E, dtype=bool)
    t_free = np.full(E, np.nan)
    status = np.full(E, DEGENERATE, dtype=np.int32)
    for e in range(E):
        if not live[e]:
            continue
        best_t, best_s = Tf[e], FREE
        for p in range(stop.shape[1]):
            tp, sp = stop[e, p], st[e, p]
            if tp < best_t or (tp == best_t and RANK[sp] < RANK[best_s]):
                best_t, best_s = tp, sp
        t_free[e], status[e] = best_t, best_s
        valid[e] = best_s == FREE
    return valid, t_free, status
