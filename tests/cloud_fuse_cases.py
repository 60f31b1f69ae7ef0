"""Inputs and references of the fused-frame tests (tests/test_cloud_fuse_host.py, tests/test_gpu_cloud_fuse.py); builds on
cloud_depth_cases.py.

``carve_ref``, ``novel_ref`` and ``append_ref`` restate the three contracts of include/nbk.h ("Fused frames") in NumPy -- the carve
one rounded float64 operation per step in the contract's order, the novelty by brute force over all pairs with the contract's
expression, the append by the two ascending lists --, and ``integrate_ref`` composes them with ``backproject_ref`` (and, with a robot,
``filter_ref``, the oracle) into what ``PointCloud.integrate_depth`` must leave in the store.  Everything here is exact: results
are compared for equality."""
import numpy as np

import cloud_depth_cases as dc

MARGIN = 0.02
WINDOWS = (0, 1, 2)
KINDS = (("f32", 1.0), ("u16", 0.001))
RAY_SCALES = (0.6, 0.85, 0.97, 1.0, 1.03, 1.3)
# the cases whose reference must carve between 5 % and 70 % of the live points: (H, W) -> windows
BANDED = {(17, 33): (0, 1, 2), (1, 64): (0,), (5, 7): (0,)}


def window_fits(H, W, window):
    return 2 * window + 1 <= min(H, W)


# ---- the surface frame ---------------------------------------------------------------------------------------------------------------
def surface_image(H, W, kind):
    """An (H, W) image of a SURFACE: a plane tilted from 1.2 m (first pixel) to 2.0 m (last), a block 0.5 m nearer over the middle
    third of the columns (and of the rows, where the image has three), and the fixed holes of ``dc.depth_image`` at pixels 1 ... 6."""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    z = 1.2 + 0.8 * (u + v) / max(W + H - 2, 1)
    block = (3 * u >= W) & (3 * u < 2 * W)
    if H >= 3:
        block &= (3 * v >= H) & (3 * v < 2 * H)
    z[block] -= 0.5
    n = H * W
    if kind == "f32":
        d = z.astype(np.float32).reshape(-1)
        holes = [np.float32(0.0), np.float32(dc.Z_MIN), np.float32(3.5), np.float32(np.nan), np.float32(np.inf), np.float32(-1.0)]
    else:
        d = np.round(z * 1000.0).astype(np.uint16).reshape(-1)
        holes = [np.uint16(0), np.uint16(250), np.uint16(3001), np.uint16(65535)]
    for k, h in enumerate(holes):
        if 1 + k < n:
            d[1 + k] = h
    return np.ascontiguousarray(d.reshape(H, W))


def stored_points(depth, intr, T, scale, seed=0):
    """The store the surface frame is carved against -> (points (M, 3), keep (M,) uint8): the frame's own back-projection scaled along
    the ray from the camera by each of RAY_SCALES with 2 mm of jitter (in front of the surface, on it, behind it), 32 points scattered
    around the camera (behind it and outside the image too), one NaN point and one infinite one; every seventh comes in released."""
    rng = np.random.default_rng(seed + 31 * depth.shape[0] + depth.shape[1])
    pts, keep = dc.backproject_ref(depth, intr, T, scale, dc.Z_MIN, dc.Z_MAX)
    seen = pts[keep != 0]
    c = np.asarray(T, dtype=np.float64)[:3, 3]
    parts = [c + s * (seen - c) + rng.uniform(-0.002, 0.002, seen.shape) for s in RAY_SCALES]
    parts.append(c + rng.uniform(-1.5, 1.5, (32, 3)))
    parts.append(np.array([[np.nan, 0.1, 0.2], [0.3, np.inf, -0.4]]))
    out = np.ascontiguousarray(np.concatenate(parts))
    k = np.ones((out.shape[0],), dtype=np.uint8)
    k[::7] = 0
    return out, k


def carve_case(H, W, kind):
    """-> (depth, intrinsics, pose (4, 4), depth_scale, stored points, stored keep) of one carve case."""
    scale = dict(KINDS)[kind]
    d = surface_image(H, W, kind)
    intr, T = dc.intrinsics(H, W), dc.camera_pose()
    pts, keep = stored_points(d, intr, T, scale)
    return d, intr, T, scale, pts, keep


def carve_ref(pts, keep, depth, intr, T, margin, window, depth_scale=1.0, z_min=0.0, z_max=np.inf):
    """The new store mask (M,) uint8 by the contract:
        d[e] = p[e] - T[e][3];  xc = (T[0][0] d[0] + T[1][0] d[1]) + T[2][0] d[2], yc and zc with columns 1 and 2;
        u = floor(((xc fx) / zc + cx) + 0.5), v = floor(((yc fy) / zc + cy) + 0.5)
    keep goes to 0 iff it was not 0, zc > z_min, the window around (u, v) lies in the image (compared as doubles) and every pixel of it
    is valid with (z_m - zc) > margin."""
    d = np.asarray(depth)
    if d.dtype == np.int16:
        d = d.view(np.uint16)
    H, W = d.shape
    fx, fy, cx, cy = (np.float64(x) for x in intr)
    T = np.asarray(T, dtype=np.float64)[:3, :4]
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    out = np.asarray(keep).astype(np.uint8).copy()
    w = np.float64(window)
    margin = np.float64(margin)
    with np.errstate(all="ignore"):
        dd = [p[:, e] - T[e, 3] for e in range(3)]
        xc, yc, zc = ((T[0, j] * dd[0] + T[1, j] * dd[1]) + T[2, j] * dd[2] for j in range(3))
        u = np.floor(((xc * fx) / zc + cx) + 0.5)
        v = np.floor(((yc * fy) / zc + cy) + 0.5)
        ok = (out != 0) & (zc > np.float64(z_min))
        ok &= (u - w >= 0.0) & (u + w <= np.float64(W - 1)) & (v - w >= 0.0) & (v + w <= np.float64(H - 1))
        zm = d.astype(np.float64) * np.float64(depth_scale)
        valid = ((zm - zm) == 0.0) & (zm > np.float64(z_min)) & (zm <= np.float64(z_max))
        idx = np.flatnonzero(ok)
        ui, vi, zi = u[idx].astype(np.int64), v[idx].astype(np.int64), zc[idx]
        through = np.ones(idx.shape, dtype=bool)
        for b in range(-window, window + 1):
            for a in range(-window, window + 1):
                through &= valid[vi + b, ui + a] & ((zm[vi + b, ui + a] - zi) > margin)
    out[idx[through]] = 0
    return out


def carved_fraction(keep_in, keep_out):
    live = np.asarray(keep_in) != 0
    return float(np.mean(np.asarray(keep_out)[live] == 0)) if live.any() else 0.0


def in_band(keep_in, keep_out, what):
    """The condition on the reference: it carves between 5 % and 70 % of the live points."""
    f = carved_fraction(keep_in, keep_out)
    assert 0.05 <= f <= 0.70, f"{what}: the reference carves {f:.3f} of the live points -- not a mixed case"
    return f


# ---- novelty -------------------------------------------------------------------------------------------------------------------------
def novel_ref(cloud_pts, pts, keep, merge):
    """The new frame mask (N,) uint8 by brute force: keep goes to 0 iff it was not 0 and some cloud point (``cloud_pts``: the ones that
    count) has ((dx dx + dy dy) + dz dz) < merge merge, dx = p[0] - c[0], ...; merge <= 0 drops nothing."""
    c = np.asarray(cloud_pts, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    out = np.asarray(keep).astype(np.uint8).copy()
    if not merge > 0.0 or c.shape[0] == 0 or p.shape[0] == 0:
        return out
    m2 = np.float64(merge) * np.float64(merge)
    hit = np.zeros((p.shape[0],), dtype=bool)
    with np.errstate(all="ignore"):
        for lo in range(0, p.shape[0], 512):
            q = p[lo:lo + 512]
            dx, dy, dz = (q[:, None, e] - c[None, :, e] for e in range(3))
            hit[lo:lo + 512] = (((dx * dx + dy * dy) + dz * dz) < m2).any(axis=1)
    out[(out != 0) & hit] = 0
    return out


# ---- append --------------------------------------------------------------------------------------------------------------------------
def append_ref(store_pts, store_keep, new_pts, new_keep):
    """-> (store_pts, store_keep, counts (3,) int64, slot_of (N,) int32) by the two ascending lists: F the free slots, A the new points
    kept; the k-th of A goes to the k-th of F for k < min(|F|, |A|)."""
    sp = np.asarray(store_pts, dtype=np.float64).copy()
    sk = np.asarray(store_keep).astype(np.uint8).copy()
    new_pts = np.asarray(new_pts, dtype=np.float64).reshape(-1, 3)
    F = np.flatnonzero(sk == 0)
    A = np.flatnonzero(np.asarray(new_keep) != 0)
    k = min(F.shape[0], A.shape[0])
    sp[F[:k]] = new_pts[A[:k]]
    sk[F[:k]] = 1
    slot_of = np.full((new_pts.shape[0],), -1, dtype=np.int32)
    slot_of[A[:k]] = F[:k]
    counts = np.array([sk.shape[0] - F.shape[0] + k, k, A.shape[0] - k], dtype=np.int64)
    return sp, sk, counts, slot_of


# ---- the whole call ------------------------------------------------------------------------------------------------------------------
def integrate_ref(store, depth, intr, T, radius, margin, window, merge, sm=None, q=None, pad=0.0, shapes=None, clear_robot=True,
                  depth_scale=1.0, z_min=0.0, z_max=np.inf):
    """One ``integrate_depth`` on ``store`` = (points (M, 3), keep (M,) uint8) -> (new store, counts, carved slots, slot_of): T is the
    OPTICAL pose; with ``sm`` (and q, pad, shapes) the two self-filter steps are the oracle's."""
    sp, sk = store
    pts, keep = dc.backproject_ref(depth, intr, T, depth_scale, z_min, z_max)
    if sm is not None:
        idx = np.flatnonzero(keep)
        keep[idx] = dc.filter_ref(sm, pts[idx], radius, q, pad, shapes)
    carved = carve_ref(sp, sk, depth, intr, T, margin, window, depth_scale, z_min, z_max)
    released = np.flatnonzero((sk != 0) & (carved == 0))
    sk = carved
    if sm is not None and clear_robot:
        idx = np.flatnonzero(sk)
        sk[idx] = dc.filter_ref(sm, sp[idx], radius, q, pad, shapes)
    keep = novel_ref(sp[sk != 0], pts, keep, merge)
    sp, sk, counts, slot_of = append_ref(sp, sk, pts, keep)
    return (sp, sk), counts, released, slot_of


def empty_store(capacity):
    return np.zeros((capacity, 3), dtype=np.float64), np.zeros((capacity,), dtype=np.uint8)


# ---- an analytic scene: a wall and a sphere in front of it ---------------------------------------------------------------------------
WALL_X = 0.6
SPHERE_C, SPHERE_R = np.array([0.1, 0.05, 0.5]), 0.15
SPHERE_MOVED = np.array([0.1, -0.35, 0.6])


def look_along_x(position, yaw=0.0, pitch=0.0):
    """The (4, 4) OPTICAL pose of a camera at ``position`` that looks along world x (z up), turned by yaw about z and pitch about y."""
    cy_, sy_, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Rz = np.array([[cy_, -sy_, 0.0], [sy_, cy_, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    cam = Rz @ Ry                                            # columns: forward (x), left (y), up (z) of the camera in the world
    T = np.eye(4)
    T[:3, :3] = np.stack((-cam[:, 1], -cam[:, 2], cam[:, 0]), axis=1)
    T[:3, 3] = position
    return T


POSES = (look_along_x([-1.2, 0.05, 0.5]), look_along_x([-1.1, -0.5, 0.65], yaw=0.35, pitch=0.1),
         look_along_x([-1.0, 0.6, 0.4], yaw=-0.4, pitch=-0.08))


def render(T, intr, H, W, sphere_c=SPHERE_C, sphere_r=SPHERE_R, wall_x=WALL_X):
    """The (H, W) float32 depth image (metric depth along the view axis; 0 where a ray meets nothing) of the wall x = wall_x and the
    sphere, by ray casting from the optical pose T."""
    fx, fy, cx, cy = intr
    R, o = np.asarray(T)[:3, :3], np.asarray(T)[:3, 3]
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack(((u - cx) / fx, (v - cy) / fy, np.ones_like(u)), axis=-1) @ R.T          # world direction per unit of depth
    with np.errstate(all="ignore"):
        z = np.where(ray[..., 0] > 1e-9, (wall_x - o[0]) / ray[..., 0], np.inf)
        oc = o - np.asarray(sphere_c)
        a = np.sum(ray * ray, axis=-1)
        b = 2.0 * (ray @ oc)
        disc = b * b - 4.0 * a * (oc @ oc - sphere_r * sphere_r)
        s = (-b - np.sqrt(disc)) / (2.0 * a)
        z = np.where((disc > 0.0) & (s > 0.0) & (s < z), s, z)
    z[~np.isfinite(z) | (z <= 0.0)] = 0.0
    return np.ascontiguousarray(z.astype(np.float32))
