"""Rendered frames, the part that needs no device (include/nbk.h: nbk_render_ray_spans_host, nbk_render_depth_lds_bytes,
nbk_render_depth_batch's argument rules; DeviceModel.render_depth's; World.depth_image's signature): the ray spans bit for bit their
NumPy restatement, the march restated on one sphere inside the bound the device tests use, and the conditions on the analytic
references those tests compare with."""
import ctypes as C
import inspect

import numpy as np
import pytest

from numbotics_amd import _lib
from numbotics_amd.physics import ray_spans_host, optical_pose
import render_cases as rc
import cloud_depth_cases as dc

INVALID = -1


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{what}: bits differ"


# balls in front of, behind, around and beside a camera at the origin of its frame (centres are given in the CAMERA frame and moved
# to the world with the pose), and one far away
BALLS_CAM = np.array([[0.1, 0.05, 1.3], [0.0, 0.0, -1.0], [0.02, -0.01, 0.03], [3.0, 0.1, 0.4], [-0.4, 0.3, 2.5], [0.0, 0.0, 40.0]])
RADII = np.array([0.15, 0.3, 0.5, 0.2, 0.6, 1.0])


@pytest.mark.parametrize("frame", ["optical", "numbotics"])
@pytest.mark.parametrize("H,W", [(1, 1), (13, 9), (36, 48)])
def test_ray_spans_equal_their_restatement_bitwise(H, W, frame):
    T = dc.camera_pose()
    To = optical_pose(T, frame)
    centres = BALLS_CAM @ To[:3, :3].T + To[:3, 3]
    intr = dc.intrinsics(H, W)
    seen = set()
    for near, far in ((0.01, 1000.0), (1.25, 2.4), (0.0, 1.2)):
        span, hit = ray_spans_host(H, W, intr, T, centres, RADII, near, far, frame=frame)
        rs, rh = rc.spans_ref(H, W, intr, To, centres, RADII, near, far)
        _bits(hit, rh, f"{W}x{H} {frame} [{near}, {far}]: hit")
        _bits(span, rs, f"{W}x{H} {frame} [{near}, {far}]: span")
        assert not hit[:, 1].any(), "a ball behind the camera has no span"
        assert hit[:, 2].all() == (near < 0.4), "the ball around the camera is met by every ray unless the near plane lies beyond it"
        if H * W > 1:
            assert (near > 1.0) or (hit[:, 0].any() and not hit[:, 0].all()), "the ball in front is met by some rays"
            assert not hit[:, 3].any(), "the ball beside the camera is outside this field of view"
        assert np.all(span[hit][:, 0] >= near) and np.all(span[hit][:, 1] <= far) and np.all(span[~hit] == 0.0)
        # an end that is not clipped lies on the ball
        u, v = rc.pixel_grid(H, W)
        for s in range(len(RADII)):
            for k in (0, 1):
                z = span[:, s, k]
                free = hit[:, s] & (z > near) & (z < far)
                p = rc.points_at(intr, To, u[free], v[free], z[free])
                assert np.all(np.abs(np.linalg.norm(p - centres[s], axis=1) - RADII[s]) < 1e-9)
                seen.add((s, k, bool(free.any())))
        clipped = hit & ((span[:, :, 0] == near) | (span[:, :, 1] == far))
        seen.add(("clipped", bool(clipped.any())))
    if H * W > 1:
        assert (0, 0, True) in seen and (0, 1, True) in seen and (4, 0, True) in seen and ("clipped", True) in seen


def test_ray_span_argument_rules():
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def call(**kw):
        a = dict(H=2, W=2, fx=30.0, fy=30.0, cx=0.5, cy=0.5, T=p, c=p, r=p, S=1, near=0.01, far=10.0, span=p, hit=p)
        a.update(kw)
        return lib.nbk_render_ray_spans_host(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], a["T"], a["c"], a["r"], a["S"], a["near"], a["far"],
                                             a["span"], a["hit"])
    assert call() == 0 and call(H=0, span=None, hit=None) == 0 and call(S=0, c=None, r=None, span=None, hit=None) == 0
    for kw in (dict(H=-1), dict(W=-1), dict(S=-1), dict(fx=0.0), dict(fy=float("nan")), dict(T=None), dict(near=-0.1), dict(far=0.01),
               dict(far=float("nan")), dict(c=None), dict(r=None), dict(span=None), dict(hit=None)):
        assert call(**kw) == INVALID, kw


def test_march_on_one_sphere_stays_inside_the_bound():
    """The renderer's march, restated with the sphere's closed-form distance: camera at the origin, fov 60, sphere r = 0.15 at
    (0.1, 0.05, 1.3), eps 1e-6.  Every hit pixel with incidence cosine >= 0.2 stops in front of the true surface, by at most
    eps / (L cos): the body lies behind its tangent plane at the hit (convexity), so a point within eps of the body is within
    eps / cos of that plane along the ray, and a unit of depth is L long.  With a bounding ball 0.05 too large (what a box or a
    link's hull has) no pixel of a 160 x 120 frame needs more than 256 steps."""
    c, r = rc.CENTRE, 0.15
    Tc = np.eye(4)
    for H, W in ((36, 48), (13, 9)):
        intr = rc.intrinsics(H, W)
        t = rc.truth(rc.SH_SPHERE, rc._pose((0, 0, 0), c), np.array([r, 0, 0, 0.0]), H, W, intr, Tc)
        for slack in (0.0, 0.05):
            z, state, steps = rc.march_sphere(H, W, intr, Tc, c, r, slack=slack)
            assert not (state == 0).any() and steps.max() <= 256
            ok = (state == 1) & t["hit"] & (t["cos"] >= 0.2)
            assert ok.sum() >= (30 if H == 36 else 2)
            err = t["z"][ok] - z[ok]
            assert np.all(err >= 0.0) and np.all(err <= (rc.EPS / (t["L"] * t["cos"]))[ok]), (err.min(), err.max())
            mism = (state == 1) != t["hit"]
            assert not (mism & ~t["graze"]).any()
    H, W = 120, 160
    z, state, steps = rc.march_sphere(H, W, rc.intrinsics(H, W), Tc, c, r, slack=0.05)
    assert not (state == 0).any() and 1 < steps.max() <= 256, steps.max()
    assert (state == 1).sum() > 400 and steps[steps > 0].mean() < 40


@pytest.mark.parametrize("case", rc.analytic_cases(), ids=[c[0] for c in rc.analytic_cases()])
def test_analytic_references_meet_their_conditions(case):
    name, kind, T, prm, far, cams = case
    intr = rc.intrinsics(rc.H1, rc.W1)
    for k, Tc in enumerate(cams):
        t = rc.truth(kind, T, prm, rc.H1, rc.W1, intr, Tc, far=far)
        rc.reference_conditions(t, f"{name} pose {k}")
        # the caster agrees with the primitive's signed distance: the hit point lies on the surface, the ray before it outside
        o, w, _ = rc.rays(rc.H1, rc.W1, intr, Tc)
        zh = t["z"][t["hit"]]
        assert np.all(np.abs(rc.sd_shape(kind, T, prm, o + zh[:, None] * w[t["hit"]])) < 1e-9)
        assert np.all(rc.sd_shape(kind, T, prm, o + (0.5 * zh)[:, None] * w[t["hit"]]) > 0.0)
        assert t["graze"].sum() <= 2


def test_render_lds_bytes_are_monotone():
    """Per selected robot shape a record of 20 doubles (the core's 19 and the bounding ball) and an entry of each of the four tiles'
    candidate lists (a mask word and an index): 208 bytes; room for one record at least."""
    f = _lib.load().nbk_render_depth_lds_bytes
    assert f(0) == 160 and f(1) == 208
    prev = f(0)
    for n in range(1, 788):
        b = f(n)
        assert b == 208 * n and b > prev and b <= 160 * 1024, n
        prev = b
    assert 208 * 788 > 160 * 1024
    for n in (788, 1024, 1 << 20, -1):
        assert f(n) == -1, n


def test_render_depth_batch_argument_rules():
    """NBK_ERR_INVALID before any device is looked for (a model handle that is never read stands for one)."""
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ok = dict(m=p, q=p, Bq=1, T=p, Bt=1, B=1, H=4, W=4, fx=30.0, fy=30.0, cx=1.5, cy=1.5, near=0.01, far=10.0, eps=1e-6, steps=256,
              bits=None, world=1, miss=0.0, depth=p, label=None, counts=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.nbk_render_depth_batch(a["m"], a["q"], a["Bq"], a["T"], a["Bt"], a["B"], a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"],
                                          a["near"], a["far"], a["eps"], a["steps"], a["bits"], a["world"], a["miss"], a["depth"], a["label"],
                                          a["counts"], None)
    nan = float("nan")
    for kw in (dict(m=None), dict(T=None), dict(depth=None), dict(H=-1), dict(W=-1), dict(B=-1), dict(fx=0.0), dict(fx=-1.0), dict(fy=nan),
               dict(eps=0.0), dict(eps=-1e-6), dict(eps=nan), dict(near=-0.01), dict(far=0.01), dict(far=0.005), dict(far=nan), dict(steps=0),
               dict(steps=4097), dict(Bq=2), dict(Bt=3), dict(B=4, Bq=2, Bt=4), dict(B=4, Bq=4, Bt=3), dict(B=1 << 27, Bq=1 << 27, Bt=1 << 27),
               dict(H=1 << 15, W=1 << 16), dict(B=2, Bq=2, Bt=2, H=1 << 15, W=1 << 15)):
        assert call(**kw) == INVALID, kw


def test_render_depth_argument_errors_need_no_device():
    """``DeviceModel.render_depth`` answers a wrong argument before it touches the device: a descriptor that was never created."""
    from numbotics_amd.engine import DeviceModel
    sm = rc.static_model([(rc.SH_SPHERE, rc._pose((0, 0, 0), rc.CENTRE), np.array([0.15, 0, 0, 0.0]))])
    dev = object.__new__(DeviceModel)
    dev.scene, dev.n_q = sm, 1
    q, T, intr = np.zeros((1, 1)), np.eye(4), rc.intrinsics(4, 4)
    for kw in (dict(near=-1.0), dict(near=2.0, far=1.0), dict(far=float("nan")), dict(eps=0.0), dict(eps=float("nan")), dict(max_steps=0),
               dict(max_steps=4097), dict(shapes=[0]), dict(frame="camera")):
        with pytest.raises(ValueError):
            dev.render_depth(q, T, intr, 4, 4, **kw)
    for bad in ((0.0, 30.0, 1.5, 1.5), (30.0, -1.0, 1.5, 1.5), (30.0, 30.0, 1.5), np.eye(2)):
        with pytest.raises(ValueError):
            dev.render_depth(q, T, bad, 4, 4)
    for h, w in ((-1, 4), (4, -1)):
        with pytest.raises(ValueError):
            dev.render_depth(q, T, intr, h, w)


def test_world_depth_image_signature_is_the_references():
    """numbotics/physics/world.py:363-371: depth_image(self, width, height, camera_pose, near=0.01, far=1000, fov=60); the shape mode
    is an extra keyword behind them."""
    from numbotics_amd.physics import World
    ps = list(inspect.signature(World.depth_image).parameters.values())
    assert [p.name for p in ps[:7]] == ["self", "width", "height", "camera_pose", "near", "far", "fov"]
    assert [p.default for p in ps[4:7]] == [0.01, 1000, 60]
    assert all(p.default is inspect.Parameter.empty for p in ps[:4])
    assert [(p.name, p.default) for p in ps[7:]] == [("bullet_margins", True)]
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in ps)


def test_public_names():
    import numbotics_amd.physics as ph
    from numbotics_amd.robots import Arm
    from numbotics_amd.engine import DeviceModel
    assert "ray_spans_host" in ph.__all__ and "optical_pose" in ph.__all__
    assert callable(Arm.depth_images) and callable(DeviceModel.render_depth) and callable(ph.World.static_scene)


def test_static_scene_holds_every_body(fresh_world):
    """``World.static_scene`` needs no device: the chain's link shapes at its configuration and the obstacles, all as world shapes."""
    from numbotics_amd.scenes import build_scene
    from numbotics_amd.engine import model_desc
    arm, chain, obs = build_scene("c2")
    sm, own = fresh_world.static_scene(), arm.scene_model()
    assert sm.n_rshapes == 0 and sm.n_pairs == 0 and sm.kin.n_joints == 0
    assert sm.n_wshapes == own.n_rshapes + own.n_wshapes == 12
    assert sorted(set(sm.wshape_obj.tolist())) == [0, 1], "two bodies: the cube and the chain"
    d, _ = model_desc(sm)
    assert d.n_wshapes == 12 and d.n_rshapes == 0
    sharp = fresh_world.static_scene(bullet_margins=False)
    assert np.all(sharp.wshape_param[:, 3] == 0.0) and np.any(sm.wshape_param[:, 3] > 0.0)
