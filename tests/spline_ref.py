"""NumPy + CPU-oracle restatement of nbk_spline_validity_batch (DiscreteConnector.validate_trajectories), for the tests.

Per trajectory: the speed bound V with the exact fused multiply-add of the C contract (``Fraction``, as tests/continuous_ref.py does),
the samples t_j = j * step (j < m), t_m = 1, the general de Boor branch of ``UnitBSpline.__call__`` vectorised over the samples, and
the verdicts of ``Oracle.validity`` (a non-finite row collides there too)."""
import math
from fractions import Fraction

import numpy as np

MIN_SPEED = 1.1920928955078125e-07          # 2^-23
DBL_MAX = 1.7976931348623157e308


def _fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    try:
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    except OverflowError:
        return math.inf


def speed_bound(ctrl, knots, k):
    """V of one trajectory: max over the legs with den_i > 0 of (k * |c[i+1] - c[i]|) / den_i, NaN when any of them is NaN."""
    n, nq = ctrl.shape
    V, nan = 0.0, False
    for i in range(n - 1):
        den = float(knots[i + k + 1] - knots[i + 1])
        if den <= 0.0:
            continue
        acc = 0.0
        for c in range(nq):
            df = float(ctrl[i + 1, c] - ctrl[i, c])
            acc = _fma(df, df, acc)
        v = (float(k) * math.sqrt(acc)) / den
        if v != v:
            nan = True
        elif v > V:
            V = v
    return math.nan if nan else V


def sample_times(ctrl, knots, k, resolution):
    """t_j of one trajectory (an empty array for a degenerate one)."""
    V = speed_bound(ctrl, knots, k)
    if not (V > MIN_SPEED and V <= DBL_MAX):
        return np.empty(0)
    step = resolution / V
    inv = 1.0 / step if step > 0.0 else math.inf
    if not inv < 2.0 ** 31:
        raise ValueError("too many samples")
    m = math.ceil(inv)
    return np.append(np.arange(m, dtype=np.float64) * step, 1.0)


def de_boor(ctrl, knots, k, sidx, t):
    """q rows of trajectories ctrl[sidx] at t (vectorised ``UnitBSpline.__call__``, general branch): ctrl (S, n, nq), sidx / t (N,)."""
    knots = np.asarray(knots, dtype=np.float64)
    n = ctrl.shape[1]
    t = np.asarray(t, dtype=np.float64)
    ell = np.clip(np.searchsorted(knots, t, side="right") - 1, k, n - 1)
    d = [ctrl[sidx, ell - k + j, :] for j in range(k + 1)]
    for r in range(1, k + 1):
        for j in range(k, r - 1, -1):
            ta = knots[j + ell - k]
            den = knots[j + 1 + ell - r] - ta
            with np.errstate(divide="ignore", invalid="ignore"):
                alpha = np.where(den == 0.0, 0.0, (t - ta) / np.where(den == 0.0, 1.0, den))
            d[j] = (1.0 - alpha)[:, None] * d[j - 1] + alpha[:, None] * d[j]
    return d[k]


def spline_samples(ctrl, knots, k, resolution):
    """(t, q) of every sample of one trajectory ctrl (n, nq)."""
    t = sample_times(ctrl, knots, k, resolution)
    return t, de_boor(ctrl[None], knots, k, np.zeros(t.shape[0], dtype=np.int64), t)


def reference_splines(orc, ctrl, knots, k, resolution, threshold=0.0, nthreads=8, chunk_rows=1 << 20):
    """-> valid (S,) bool, t_hit (S,), n_samples (S,) int32 of nbk_spline_validity_batch."""
    ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
    knots = np.asarray(knots, dtype=np.float64)
    S = ctrl.shape[0]
    times = [sample_times(ctrl[s], knots, k, resolution) for s in range(S)]
    ns = np.array([t.shape[0] for t in times], dtype=np.int32)
    valid = np.zeros(S, dtype=bool)
    t_hit = np.full(S, np.nan)
    s0 = 0
    while s0 < S:                                   # trajectories in groups of about chunk_rows samples
        s1, rows = s0, 0
        while s1 < S and (s1 == s0 or rows + ns[s1] <= chunk_rows):
            rows += int(ns[s1])
            s1 += 1
        if rows > 0:
            sidx = np.repeat(np.arange(s0, s1), ns[s0:s1])
            t = np.concatenate(times[s0:s1])
            hit = orc.validity(de_boor(ctrl, knots, k, sidx, t), threshold, nthreads=nthreads)
            o = 0
            for s in range(s0, s1):
                h = hit[o:o + ns[s]]
                if ns[s] > 0:
                    j = np.flatnonzero(h)
                    valid[s] = j.size == 0
                    if j.size:
                        t_hit[s] = times[s][j[0]]
                o += int(ns[s])
        s0 = s1
    return valid, t_hit, ns


def random_splines(chain, S, n, seed, near=None, spread=0.25):
    """S trajectories of n control points: half spread over the joint box, half clustered within `spread` of `near` (a free
    configuration, when given)."""
    rng = np.random.default_rng(seed)
    lim = np.asarray(chain.joint_limits, dtype=np.float64)
    lim = np.where(np.isfinite(lim), lim, np.sign(lim) * np.pi)
    c = rng.uniform(lim[:, 0], lim[:, 1], (S, n, chain.dof))
    if near is not None:
        h = S // 2
        c[h:] = near + rng.uniform(-spread, spread, (S - h, n, chain.dof))
    return c
