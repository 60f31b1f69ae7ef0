"""Inputs and the reference of the point-cloud tests (tests/test_gpu_cloud.py; tools/cloud_time.py draws its clouds with ``scan``).

The reference is the CPU oracle as it is: a cloud of N points of radius r equals N sphere world shapes of radius r, paired with the
selected robot shapes -- ``cloud_model`` builds that SceneModel; pair p of it is (shapes[p // N], point p % N)."""
import dataclasses

import numpy as np

SH_SPHERE = 0


def scan(n, seed=0):
    """The "scan": the first n // 2 points on a wall x = 0.45, y ~ U(-0.5, 0.5), z ~ U(0, 1), the rest on a table z = 0.10,
    x, y ~ U(-0.6, 0.6)."""
    rng = np.random.default_rng(seed)
    w = n // 2
    pts = np.empty((n, 3))
    pts[:w, 0] = 0.45
    pts[:w, 1] = rng.uniform(-0.5, 0.5, w)
    pts[:w, 2] = rng.uniform(0.0, 1.0, w)
    pts[w:, 0] = rng.uniform(-0.6, 0.6, n - w)
    pts[w:, 1] = rng.uniform(-0.6, 0.6, n - w)
    pts[w:, 2] = 0.10
    return pts


def cloud_model(sm, pts, r, shapes=None, keep_scene=False):
    """``sm`` with the cloud as its world: N sphere world shapes (identity rotation, translation p_i, param[0] = r) and the pairs
    (s, point) for s in ``shapes`` (default: every robot shape), shape-major.  ``keep_scene``: keep sm's own world shapes and pairs
    in front of the cloud's (the combined model of the accumulate test; cloud pair p is then at sm.n_pairs + p)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    N = pts.shape[0]
    S = sm.n_rshapes
    shapes = np.arange(S, dtype=np.int32) if shapes is None else np.asarray(sorted(shapes), dtype=np.int32)
    pose = np.zeros((N, 3, 4))
    pose[:, 0, 0] = pose[:, 1, 1] = pose[:, 2, 2] = 1.0
    pose[:, :, 3] = pts
    param = np.zeros((N, 4))
    param[:, 0] = r
    W0 = sm.n_wshapes if keep_scene else 0
    pa = np.repeat(shapes, N).astype(np.int32)
    pb = (S + W0 + np.tile(np.arange(N, dtype=np.int32), shapes.shape[0])).astype(np.int32)
    wt, wp, wq = np.zeros((N,), dtype=np.int32) + SH_SPHERE, pose.reshape(N, 12), param
    wo = np.zeros((N,), dtype=np.int32)
    if keep_scene:
        # the arm's own pairs first, then the cloud's: NOT sorted by pair_a -- the oracle takes pairs in the order given
        wt = np.concatenate((sm.wshape_type, wt)); wp = np.concatenate((sm.wshape_pose, wp)); wq = np.concatenate((sm.wshape_param, wq))
        wo = np.concatenate((sm.wshape_obj, wo))
        pa = np.concatenate((sm.pair_a, pa)); pb = np.concatenate((sm.pair_b, pb))
    return dataclasses.replace(sm, wshape_type=wt.astype(np.int32), wshape_pose=np.ascontiguousarray(wp), wshape_param=np.ascontiguousarray(wq),
                               wshape_obj=wo.astype(np.int32), pair_a=pa.astype(np.int32), pair_b=pb.astype(np.int32))


def cloud_mask(sm, pts, r, q, thr, shapes=None):
    """The oracle's verdicts of q against the cloud; all free for an empty cloud or an empty selection (the oracle needs a pair)."""
    from oracle.cpu_oracle import Oracle
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1, sm.kin.n_q)
    if pts.shape[0] == 0 or (shapes is not None and len(shapes) == 0):
        return np.zeros((q.shape[0],), dtype=bool)
    return Oracle(cloud_model(sm, pts, r, shapes)).validity(q, thr)


def cloud_closest(sm, pts, r, q, d_max, shapes=None):
    """(distance, shape, point) of the oracle's closest pair per row, cut at d_max: +inf, -1, -1 where the minimum is >= d_max."""
    from oracle.cpu_oracle import Oracle
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1, sm.kin.n_q)
    N = pts.shape[0]
    sel = np.arange(sm.n_rshapes, dtype=np.int32) if shapes is None else np.asarray(sorted(shapes), dtype=np.int32)
    if N == 0 or sel.shape[0] == 0:
        return np.full((q.shape[0],), np.inf), np.full((q.shape[0],), -1, dtype=np.int32), np.full((q.shape[0],), -1, dtype=np.int32)
    d, p = Oracle(cloud_model(sm, pts, r, shapes)).closest(q)
    near = d < d_max
    return (np.where(near, d, np.inf), np.where(near, sel[p // N], -1).astype(np.int32), np.where(near, p % N, -1).astype(np.int32))


def pack_bits(mask):
    """(B,) bool -> (ceil(B / 64),) int64 words, bit b % 64 of word b // 64."""
    mask = np.asarray(mask, dtype=bool)
    B = mask.shape[0]
    padded = np.zeros((((B + 63) // 64) * 64,), dtype=np.uint8)
    padded[:B] = mask
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1).astype(np.uint64).view(np.int64)
