"""Scenes, analytic ray casters and restatements of the rendered-frame tests (tests/test_render_host.py, tests/test_gpu_render.py).

``spans_ref`` restates the ray-span contract of numbotics_amd/csrc/nbk_cloud_depth.hpp in NumPy, one rounded float64 operation per
step, in the contract's order; ``march_sphere`` restates the renderer's march (include/nbk.h, "Rendered frames") on one sphere, whose
exact distance is a closed form.  The analytic casters intersect a ray with each primitive by its own formula; ``truth`` adds the
incidence cosine and, by a search on the primitive's signed distance along the ray (convex for a convex body), how far the ray is
from grazing it.  Everything is in WORLD coordinates with the ray p(z) = o + z w: o the camera, w the ray per unit of depth."""
import numpy as np

SH_SPHERE, SH_CAPSULE, SH_BOX, SH_CYLINDER, SH_PLANE = 0, 1, 2, 3, 4
EPS = 1e-6
NEAR, FAR = 0.01, 1000.0
FOV = 60.0


def widen(R):
    """The bounding ball the renderer takes a shape's candidates with: 1e-6 relative + 1e-7."""
    return R + (1e-6 * abs(R) + 1e-7)


def look_at(eye, target, roll=0.0):
    """An optical pose (4, 4) at ``eye`` whose z axis points at ``target``; x right, y down, turned by ``roll`` about z."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(z, up); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = c * x + s * y, -s * x + c * y, z, eye
    return T


def numbotics_pose(T_opt):
    """The reference's camera pose (x forward, z up) whose optical pose is ``T_opt``: x_cam = z, y_cam = -x, z_cam = -y."""
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = T_opt[:3, 2], -T_opt[:3, 0], -T_opt[:3, 1], T_opt[:3, 3]
    return T


def pixel_grid(H, W):
    u = np.tile(np.arange(W, dtype=np.float64), H)
    v = np.repeat(np.arange(H, dtype=np.float64), W)
    return u, v


def rays(H, W, intr, T):
    """-> (o (3,), w (H * W, 3) the world ray per unit of depth, L (H * W,)) in the contract's operand order."""
    fx, fy, cx, cy = (np.float64(x) for x in intr)
    T = np.asarray(T, dtype=np.float64)[:3, :4]
    u, v = pixel_grid(H, W)
    ax, ay = (u - cx) / fx, (v - cy) / fy
    L = np.sqrt((ax * ax + ay * ay) + 1.0)
    w = np.stack([(T[e, 0] * ax + T[e, 1] * ay) + T[e, 2] for e in range(3)], axis=1)
    return T[:, 3].copy(), w, L


def points_at(intr, T, u, v, z):
    """The march point of pixels (u, v) at depths z: the back-projection's arithmetic with depth_scale 1."""
    fx, fy, cx, cy = (np.float64(x) for x in intr)
    T = np.asarray(T, dtype=np.float64)[:3, :4]
    xc = ((u - cx) * z) / fx
    yc = ((v - cy) * z) / fy
    return np.stack([((T[e, 0] * xc + T[e, 1] * yc) + T[e, 2] * z) + T[e, 3] for e in range(3)], axis=-1)


def spans_ref(H, W, intr, T, centres, radii, near, far):
    """(span (H * W, S, 2), hit (H * W, S) bool) by the contract of nbk_cloud_depth.hpp, operation by operation."""
    fx, fy, cx, cy = (np.float64(x) for x in intr)
    T = np.asarray(T, dtype=np.float64)[:3, :4]
    u, v = pixel_grid(H, W)
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(radii, dtype=np.float64).reshape(-1)
    n, S = H * W, c.shape[0]
    span = np.zeros((n, S, 2))
    hit = np.zeros((n, S), dtype=bool)
    with np.errstate(all="ignore"):
        ax, ay = (u - cx) / fx, (v - cy) / fy
        A = (ax * ax + ay * ay) + 1.0
        for s in range(S):
            d0, d1, d2 = c[s, 0] - T[0, 3], c[s, 1] - T[1, 3], c[s, 2] - T[2, 3]
            xc = (T[0, 0] * d0 + T[1, 0] * d1) + T[2, 0] * d2
            yc = (T[0, 1] * d0 + T[1, 1] * d1) + T[2, 1] * d2
            zc = (T[0, 2] * d0 + T[1, 2] * d1) + T[2, 2] * d2
            B = (ax * xc + ay * yc) + zc
            C = ((xc * xc + yc * yc) + zc * zc) - R[s] * R[s]
            D = B * B - A * C
            ok = D >= 0.0
            sq = np.sqrt(np.where(ok, D, 0.0))
            z0 = (B - sq) / A
            z1 = (B + sq) / A
            z0 = np.where(z0 > near, z0, np.float64(near))
            z1 = np.where(z1 < far, z1, np.float64(far))
            ok = ok & (z0 <= z1)
            hit[:, s] = ok
            span[:, s, 0] = np.where(ok, z0, 0.0)
            span[:, s, 1] = np.where(ok, z1, 0.0)
    return span, hit


def march_sphere(H, W, intr, T, c, r, eps=EPS, max_steps=256, near=NEAR, far=FAR, slack=0.0):
    """The renderer's march on ONE sphere (c, r) whose bounding ball is taken ``slack`` too large (a sphere's own is exact; other kinds'
    are not): candidates by the span of the widened ball, z from z0, d = |p(z) - c| - r, hit when d < eps, else z += d / L, a miss past
    z1.  -> (z (H * W,), state (H * W,): 1 hit, 2 miss, 0 unresolved, steps (H * W,))."""
    c = np.asarray(c, dtype=np.float64)
    u, v = pixel_grid(H, W)
    _, _, L = rays(H, W, intr, T)
    span, has = spans_ref(H, W, intr, T, c.reshape(1, 3), [widen(r + slack)], near, far)
    z = np.where(has[:, 0], span[:, 0, 0], np.inf)
    z1 = span[:, 0, 1]
    state = np.where(has[:, 0], 0, 2)
    steps = np.zeros(H * W, dtype=np.int64)
    for _ in range(max_steps):
        act = state == 0
        if not act.any():
            break
        za = np.where(act, z, 0.0)
        p = points_at(intr, T, u, v, za)
        d = np.sqrt(((p - c) ** 2).sum(-1)) - r
        steps[act] += 1
        h = act & (d < eps)
        state[h] = 1
        go = act & ~h
        z = np.where(go, z + d / L, z)
        state[go & ~(z <= z1)] = 2
    return z, state, steps


# ---- the primitives: signed distance and the first intersection of a ray ----------------------------------------------------------------
def _local(T, p):
    return (p - T[:3, 3]) @ T[:3, :3]


def sd_shape(kind, T, prm, p):
    """Signed distance of world points p (..., 3) to the SHARP primitive (type, 4x4 pose, params as robots/model.py has them)."""
    if kind == SH_PLANE:
        return (p - T[:3, 3]) @ prm[:3]
    q = _local(T, p)
    if kind == SH_SPHERE:
        return np.sqrt((q * q).sum(-1)) - prm[0]
    if kind == SH_CAPSULE:
        zc = np.clip(q[..., 2], -prm[1], prm[1])
        return np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2 + (q[..., 2] - zc) ** 2) - prm[0]
    if kind == SH_BOX:
        e = np.abs(q) - prm[:3]
        return np.sqrt((np.maximum(e, 0.0) ** 2).sum(-1)) + np.minimum(e.max(-1), 0.0)
    if kind == SH_CYLINDER:
        e = np.stack((np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - prm[0], np.abs(q[..., 2]) - prm[1]), -1)
        return np.sqrt((np.maximum(e, 0.0) ** 2).sum(-1)) + np.minimum(e.max(-1), 0.0)
    raise ValueError(kind)


def _quad_entry(a, b, c):
    """The smaller root of a t^2 + 2 b t + c = 0 (a > 0), inf without one."""
    with np.errstate(all="ignore"):
        D = b * b - a * c
        return np.where(D > 0.0, (-b - np.sqrt(np.abs(D))) / a, np.inf)


def cast_shape(kind, T, prm, o, w):
    """The depth z > 0 at which the ray o + z w ENTERS the sharp primitive (the camera is outside), inf for a miss."""
    with np.errstate(all="ignore"):
        if kind == SH_PLANE:
            n = prm[:3]
            den, h = w @ n, (o - T[:3, 3]) @ n
            return np.where(den < 0.0, h / -den, np.inf)
        ol, wl = _local(T, o), w @ T[:3, :3]
        if kind == SH_SPHERE:
            z = _quad_entry((wl * wl).sum(-1), wl @ ol, ol @ ol - prm[0] ** 2)
        elif kind == SH_BOX:
            t1, t2 = (-prm[:3] - ol) / wl, (prm[:3] - ol) / wl
            lo, hi = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
            z = np.where(lo <= hi, lo, np.inf)
        else:
            r, h = prm[0], prm[1]
            side = _quad_entry(wl[:, 0] ** 2 + wl[:, 1] ** 2, wl[:, 0] * ol[0] + wl[:, 1] * ol[1], ol[0] ** 2 + ol[1] ** 2 - r * r)
            zs = ol[2] + side * wl[:, 2]
            z = np.where(np.abs(zs) <= h, side, np.inf)
            for sg in (1.0, -1.0):
                if kind == SH_CYLINDER:                  # the cap the ray can enter through: the one it moves against
                    t = (sg * h - ol[2]) / wl[:, 2]
                    x, y = ol[0] + t * wl[:, 0], ol[1] + t * wl[:, 1]
                    ok = (sg * wl[:, 2] < 0.0) & (x * x + y * y <= r * r)
                else:                                    # the capsule's end ball, on its own side of the segment's end
                    oc = ol - np.array([0.0, 0.0, sg * h])
                    t = _quad_entry((wl * wl).sum(-1), wl @ oc, oc @ oc - r * r)
                    ok = sg * (ol[2] + t * wl[:, 2]) >= h
                z = np.minimum(z, np.where(ok, t, np.inf))
        return np.where(z > 0.0, z, np.inf)


def truth(kind, T, prm, H, W, intr, Tc, near=NEAR, far=FAR, eps=EPS):
    """The analytic frame of one primitive from the optical pose Tc -> dict: z (inf: miss), hit, cos (the incidence cosine at the
    hit), L, graze (the ray's closest approach to the surface -- outside or inside -- is within 2 eps: its class is not compared)."""
    T, prm = np.asarray(T, dtype=np.float64), np.asarray(prm, dtype=np.float64)
    o, w, L = rays(H, W, intr, Tc)
    z = cast_shape(kind, T, prm, o, w)
    z = np.where((z >= near) & (z <= far), z, np.inf)
    hit = np.isfinite(z)
    zh = np.where(hit, z, 1.0)
    p = o + zh[:, None] * w
    g = np.stack([(sd_shape(kind, T, prm, p + d) - sd_shape(kind, T, prm, p - d)) / 2e-6 for d in 1e-6 * np.eye(3)], axis=1)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    cos = np.where(hit, -(g * w).sum(-1) / L, np.nan)
    if kind == SH_PLANE:
        graze = np.abs(w @ prm[:3]) < 1e-9
    else:
        lo, hi = np.full(H * W, near), np.full(H * W, min(far, 50.0))
        for _ in range(120):                             # the minimum of a convex function of z
            m1, m2 = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
            f1, f2 = sd_shape(kind, T, prm, o + m1[:, None] * w), sd_shape(kind, T, prm, o + m2[:, None] * w)
            lo, hi = np.where(f1 > f2, m1, lo), np.where(f1 > f2, hi, m2)
        graze = np.abs(sd_shape(kind, T, prm, o + (0.5 * (lo + hi))[:, None] * w)) < 2.0 * eps
    return dict(z=z, hit=hit, cos=cos, L=L, graze=graze)


def reference_conditions(t, what):
    """What every analytic case must satisfy before anything is compared with it: at least 30 hit and 30 miss pixels, at most 10 %
    of the hits below an incidence cosine of 0.2."""
    nh, nm = int(t["hit"].sum()), int((~t["hit"]).sum())
    assert nh >= 30 and nm >= 30, f"{what}: {nh} hit and {nm} miss pixels"
    low = float(np.mean(t["cos"][t["hit"]] < 0.2))
    assert low <= 0.10, f"{what}: {low:.3f} of the hits below cos 0.2"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
H1, W1 = 36, 48
CENTRE = np.array([0.1, 0.05, 1.3])


def _pose(rot, t):
    from numpy import cos, sin
    a, b, c = rot
    Rx = np.array([[1, 0, 0], [0, cos(a), -sin(a)], [0, sin(a), cos(a)]])
    Ry = np.array([[cos(b), 0, sin(b)], [0, 1, 0], [-sin(b), 0, cos(b)]])
    Rz = np.array([[cos(c), -sin(c), 0], [sin(c), cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def analytic_cases():
    """[(name, type, 4x4 pose, params, far, [two optical camera poses])]: each primitive alone, sharp."""
    cams = [np.eye(4), look_at([0.95, -0.7, 0.75], CENTRE, roll=0.4)]
    body = _pose((0.4, -0.3, 0.9), CENTRE)
    up = np.array([0.0, 0.0, 1.0])
    ground = np.eye(4)
    ground[:3, 3] = [0.0, 0.0, -1.0]
    # the ground one metre below two cameras that look 20 and 35 degrees down, clipped at far = 3: the rays near the horizon miss
    gcams = [look_at([0.0, 0.0, 0.0], [np.cos(a), 0.2, -np.sin(a)], roll=r) for a, r in ((np.deg2rad(20.0), 0.0), (np.deg2rad(35.0), 0.3))]
    return [
        ("sphere", SH_SPHERE, _pose((0, 0, 0), CENTRE), np.array([0.15, 0, 0, 0.0]), FAR, cams),
        ("capsule", SH_CAPSULE, body, np.array([0.10, 0.20, 0, 0.0]), FAR, cams),
        ("box", SH_BOX, body, np.array([0.16, 0.10, 0.20, 0.0]), FAR, cams),
        ("cylinder", SH_CYLINDER, body, np.array([0.13, 0.18, 0, 0.0]), FAR, cams),
        ("plane", SH_PLANE, ground, np.array([up[0], up[1], up[2], 0.0]), 3.0, gcams),
    ]


def intrinsics(H, W):
    from numbotics_amd.physics import intrinsics_from_fov
    return intrinsics_from_fov(W, H, FOV)


def static_model(records):
    """The zero-joint scene that holds ``records`` [(type, pose, params)] as its world shapes."""
    from numbotics_amd.physics.world import static_scene_model
    return static_scene_model(records)


# ---- the arm among its obstacles ----------------------------------------------------------------------------------------------------------
H2, W2 = 18, 24


def arm_camera(k=0):
    """Optical poses around the c2 scene, looking at the arm's middle."""
    eyes = ([1.5, 0.4, 0.9], [0.3, -1.6, 0.7], [-1.2, 0.9, 1.4])
    return look_at(eyes[k % 3], [0.0, 0.0, 0.45], roll=0.1 * k)


def robot_view(sm, q, k=1.3, direction=(0.7, 0.5, 0.45)):
    """An optical pose that looks at the middle of the robot's shape centres at q from k times their spread away."""
    import cloud_ladder_cases as clc
    ctr = clc.shape_centres(sm, np.asarray(q, dtype=np.float64)[None], list(range(sm.n_rshapes)))[0]
    tgt = ctr.mean(0)
    rad = np.linalg.norm(ctr - tgt, axis=1).max() + 0.1
    d = np.asarray(direction, dtype=np.float64)
    return look_at(tgt + k * rad * d / np.linalg.norm(d), tgt, roll=0.2)


def point_world_model(sm, pts):
    """The oracle's model of points (N, 3) as radius-0 spheres against the WORLD shapes of ``sm``: a zero-joint scene whose robot
    shapes are the points and whose pairs are (point i, world shape w), point-major -- pair_distances gives [1, N * W]."""
    import dataclasses
    from numbotics_amd.robots.model import KinematicModel, _T34
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    N, Wn = pts.shape[0], sm.n_wshapes
    z = np.zeros
    kin = KinematicModel(n_q=1, joint_parent=z(0, dtype=np.int32), joint_type=z(0, dtype=np.int32), joint_qidx=z(0, dtype=np.int32),
                         joint_offset=z((0, 12)), joint_axis=z((0, 3)), joint_rot=z((0, 27)), joint_trans=z((0, 3)), joint_slide=z((0, 3)),
                         base_pose=_T34(np.eye(4)))
    loc = np.zeros((N, 3, 4))
    loc[:, 0, 0] = loc[:, 1, 1] = loc[:, 2, 2] = 1.0
    loc[:, :, 3] = pts
    return dataclasses.replace(sm, kin=kin, rshape_frame=np.full(N, -1, dtype=np.int32), rshape_type=z(N, dtype=np.int32),
                               rshape_local=np.ascontiguousarray(loc.reshape(N, 12)), rshape_param=z((N, 4)), rshape_link=z(N, dtype=np.int32),
                               pair_a=np.repeat(np.arange(N, dtype=np.int32), Wn), pair_b=(N + np.tile(np.arange(Wn, dtype=np.int32), N)).astype(np.int32))


def oracle_distances(sm, q, pts):
    """Signed distances (N, S + W) by the CPU oracle from the points (radius-0 spheres) to every robot shape of ``sm`` at q and
    every world shape, in label order."""
    from oracle.cpu_oracle import Oracle
    from cloud_cases import cloud_model
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    N, S, Wn = pts.shape[0], sm.n_rshapes, sm.n_wshapes
    out = np.empty((N, S + Wn))
    out[:, :S] = Oracle(cloud_model(sm, pts, 0.0)).pair_distances(np.asarray(q, dtype=np.float64).reshape(1, -1)).reshape(S, N).T
    if Wn > 0:
        out[:, S:] = Oracle(point_world_model(sm, pts)).pair_distances(np.zeros((1, 1))).reshape(N, Wn)
    return out
