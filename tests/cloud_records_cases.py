"""The reference of the cloud proximity records (tests/test_cloud_records_host.py, tests/test_gpu_cloud_records.py): the CPU oracle
as it is, on ``cloud_model`` of tests/cloud_cases.py -- the cloud's points as sphere world shapes paired with the selected robot
shapes, shape-major, so pair p is (shapes[p // N], point p % N).

``raw`` runs the oracle once; ``cut`` turns its arrays into the records of one call (d_max, per configuration or per shape), so the
oracle's result is shared by every d_max and both modes of a case and is never changed."""
import numpy as np

from cloud_cases import cloud_model


class Raw:
    """dist (B, n_sel, N), wit (B, n_sel, N, 9), rows (B, n_sel, N, n_q) of the oracle; sel (n_sel,) the shapes of the columns;
    finite (B,): the rows of q without a non-finite value."""

    def __init__(self, sm, pts, r, q, shapes=None):
        from oracle.cpu_oracle import Oracle
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        q = np.asarray(q, dtype=np.float64).reshape(-1, sm.kin.n_q)
        self.n_q = sm.kin.n_q
        self.sel = np.arange(sm.n_rshapes, dtype=np.int32) if shapes is None else np.asarray(sorted(set(shapes)), dtype=np.int32)
        self.B, self.N, self.S = q.shape[0], pts.shape[0], self.sel.shape[0]
        self.finite = np.isfinite(q).all(axis=1)
        B, S, N = self.B, self.S, self.N
        if S * N == 0:                                        # (the oracle needs a pair)
            self.dist, self.wit, self.rows = np.zeros((B, S, N)), np.zeros((B, S, N, 9)), np.zeros((B, S, N, self.n_q))
            return
        d, w, j = Oracle(cloud_model(sm, pts, r, self.sel)).proximity_jacobian(np.where(self.finite[:, None], q, 0.0))
        self.dist, self.wit, self.rows = d.reshape(B, S, N), w.reshape(B, S, N, 9), j.reshape(B, S, N, self.n_q)


def _pick(raw, dist, shape, point, win, lead):
    """The records of the winners win = (b, shape column, point) index arrays, of shape ``lead``, cut and filled."""
    near = dist < np.inf
    wit = np.full(lead + (9,), np.nan)
    rows = np.zeros(lead + (raw.n_q,))
    if win is not None:
        wit[near] = raw.wit[win][near]
        rows[near] = raw.rows[win][near]
    bad = np.broadcast_to(~raw.finite.reshape((-1,) + (1,) * (len(lead) - 1)), lead)
    dist = np.where(bad, np.nan, dist)
    shape = np.where(bad | ~near, -1, shape).astype(np.int32)
    point = np.where(bad | ~near, -1, point).astype(np.int32)
    wit[bad] = np.nan
    rows[bad] = np.nan
    return dist, shape, point, wit, rows


def cut(raw, d_max, per_shape=False):
    """(dist, shape, point, witness, rows) as the device call documents them.  The winner is np.argmin in shape-major pair order:
    its first occurrence is the smallest shape, then the smallest point."""
    B, S, N = raw.B, raw.S, raw.N
    b = np.arange(B)
    if per_shape:
        lead = (B, S)
        if S == 0 or N == 0:
            z = np.zeros(lead, dtype=np.int64)
            return _pick(raw, np.full(lead, np.inf), z - 1, z - 1, None, lead)          # (S == 0: empty arrays)
        i = np.argmin(raw.dist, axis=2)                                          # (B, S)
        col = np.broadcast_to(np.arange(S)[None, :], lead)
        win = (np.broadcast_to(b[:, None], lead), col, i)
        d = raw.dist[win]
        return _pick(raw, np.where(d < d_max, d, np.inf), np.broadcast_to(raw.sel[None, :], lead), i, win, lead)
    lead = (B,)
    if S == 0 or N == 0:
        z = np.zeros(lead, dtype=np.int64)
        return _pick(raw, np.full(lead, np.inf), z - 1, z - 1, None, lead)
    p = np.argmin(raw.dist.reshape(B, S * N), axis=1)
    win = (b, p // N, p % N)
    d = raw.dist[win]
    return _pick(raw, np.where(d < d_max, d, np.inf), raw.sel[p // N], p % N, win, lead)


def second_gap(raw):
    """(B, S): how much farther the second-nearest point of each (configuration, shape) is than the nearest."""
    part = np.partition(raw.dist, 1, axis=2)
    return part[:, :, 1] - part[:, :, 0]
