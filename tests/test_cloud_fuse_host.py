"""Fused frames, the part that needs no device (include/nbk.h: nbk_frame_cloud_carve*, nbk_frame_cloud_novel, nbk_frame_cloud_append*): the
carve's arithmetic on the host against its NumPy restatement, bit for bit, on a surface with stored points in front of it, on it and
behind it; the argument rules of the five entries; and the references' own sanity (tests/cloud_fuse_cases.py)."""
import os
import re

import numpy as np
import pytest

import cloud_depth_cases as dc
import cloud_fuse_cases as fc
from conftest import ROOT
from numbotics_amd import _lib
from numbotics_amd.physics.pointcloud import carve_host

INVALID = -1
NEW = ("nbk_frame_cloud_carve", "nbk_frame_cloud_carve_host", "nbk_frame_cloud_novel", "nbk_frame_cloud_append_workspace_bytes",
       "nbk_frame_cloud_append")


@pytest.mark.parametrize("kind", [k for k, _ in fc.KINDS])
@pytest.mark.parametrize("H,W", dc.SHAPES, ids=[f"{w}x{h}" for h, w in dc.SHAPES])
def test_carve_host_is_the_restatement(H, W, kind):
    d, intr, T, scale, pts, keep = fc.carve_case(H, W, kind)
    assert keep[0] == 0 and keep[7] == 0 and keep[1] == 1 and np.isnan(pts[-2, 0]) and np.isinf(pts[-1, 1])
    seen = set()
    for window in fc.WINDOWS:
        ref = fc.carve_ref(pts, keep, d, intr, T, fc.MARGIN, window, scale, dc.Z_MIN, dc.Z_MAX)
        what = f"{W}x{H} {kind} window {window}"
        f = fc.carved_fraction(keep, ref)
        print(f"{what}: the reference carves {f:.3f} of {int((keep != 0).sum())} live points")
        if window in fc.BANDED.get((H, W), ()):
            fc.in_band(keep, ref, what)
        if not fc.window_fits(H, W, window):
            assert f == 0.0, f"{what}: the window does not fit the image, yet the reference carves"
        got = carve_host(pts, keep, d, intr, T, fc.MARGIN, window, depth_scale=scale, z_min=dc.Z_MIN, z_max=dc.Z_MAX)
        assert got.dtype == np.uint8 and got.shape == keep.shape
        assert got.tobytes() == ref.tobytes(), f"{what}: differs at {np.flatnonzero(got != ref)[:8]}"
        assert not got[keep == 0].any() and got[-2] == keep[-2] and got[-1] == keep[-1], "released, NaN and infinite points stay as they are"
        seen.add(round(f, 6))
    if (H, W) == (17, 33):
        assert len(seen) == 3, f"the window matters: {seen}"


def test_carve_reference_by_hand():
    """Three stored points on the axis of a camera at the origin that sees a flat wall at 2 m: 1 m (seen through), 1.99 m (inside the
    margin) and 2.5 m (occluded); then a hole beside the centre pixel protects the first one at window 1 and not at window 0."""
    d = np.full((3, 3), 2.0, dtype=np.float32)
    intr, T = (2.0, 2.0, 1.0, 1.0), np.eye(4)
    pts = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.99], [0.0, 0.0, 2.5], [0.0, 0.0, -1.0], [5.0, 0.0, 1.0]])
    keep = np.ones((5,), dtype=np.uint8)
    for w in (0, 1):
        assert fc.carve_ref(pts, keep, d, intr, T, 0.05, w).tolist() == [0, 1, 1, 1, 1]
        assert carve_host(pts, keep, d, intr, T, 0.05, w).tolist() == [0, 1, 1, 1, 1]
    d[0, 0] = 0.0
    assert carve_host(pts, keep, d, intr, T, 0.05, 0).tolist() == [0, 1, 1, 1, 1]
    assert carve_host(pts, keep, d, intr, T, 0.05, 1).tolist() == [1, 1, 1, 1, 1]
    assert fc.carve_ref(pts, keep, d, intr, T, 0.05, 1).tolist() == [1, 1, 1, 1, 1]
    # the comparison with the margin is strict
    d[:] = 2.0
    near = np.array([[0.0, 0.0, 1.5]])
    assert carve_host(near, [1], d, intr, T, 0.5, 0).tolist() == [1] and carve_host(near, [1], d, intr, T, 0.4375, 0).tolist() == [0]


def test_novel_and_append_references_by_hand():
    c = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    p = np.array([[0.03125, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.03, 0.0], [0.5, 0.0, 0.0], [np.nan, 0.0, 0.0]])
    assert fc.novel_ref(c, p, np.ones(5, np.uint8), 0.03125).tolist() == [1, 0, 0, 1, 1]
    assert fc.novel_ref(c, p, np.array([1, 0, 1, 1, 1], np.uint8), 0.0).tolist() == [1, 0, 1, 1, 1]
    assert fc.novel_ref(c[:0], p, np.ones(5, np.uint8), 1.0).tolist() == [1, 1, 1, 1, 1]
    sp = np.arange(15, dtype=np.float64).reshape(5, 3)
    sk = np.array([1, 0, 1, 0, 0], dtype=np.uint8)
    new = -np.arange(1, 13, dtype=np.float64).reshape(4, 3)
    a, b, counts, slot_of = fc.append_ref(sp, sk, new, [0, 1, 1, 0])
    assert b.tolist() == [1, 1, 1, 1, 0] and counts.tolist() == [4, 2, 0] and slot_of.tolist() == [-1, 1, 3, -1]
    assert np.array_equal(a[1], new[1]) and np.array_equal(a[3], new[2]) and np.array_equal(a[[0, 2, 4]], sp[[0, 2, 4]])
    a, b, counts, slot_of = fc.append_ref(sp, [1, 1, 1, 0, 1], new, [1, 1, 1, 1])
    assert b.tolist() == [1] * 5 and counts.tolist() == [5, 1, 3] and slot_of.tolist() == [3, -1, -1, -1]


def test_argument_rules_need_no_device():
    lib = _lib.load()
    buf = np.zeros((64,), dtype=np.float64)            # stands for any non-null pointer: no rule below reads through one
    p = buf.ctypes.data
    nan, inf = float("nan"), float("inf")
    ok = dict(depth=p, depth_type=0, H=2, W=3, scale=1.0, fx=1.0, fy=1.0, cx=0.0, cy=0.0, T=p, z_min=0.0, z_max=1.0, margin=0.02, window=1,
              pts=p, M=4, keep=p)

    def cv(host, **kw):
        a = dict(ok, **kw)
        args = [a["depth"], a["depth_type"], a["H"], a["W"], a["scale"], a["fx"], a["fy"], a["cx"], a["cy"], a["T"], a["z_min"], a["z_max"],
                a["margin"], a["window"], a["pts"], a["M"], a["keep"]]
        return lib.nbk_frame_cloud_carve_host(*args) if host else lib.nbk_frame_cloud_carve(*(args + [None]))

    bad = [dict(depth=None), dict(T=None), dict(pts=None), dict(keep=None), dict(H=-1), dict(W=-1), dict(H=4097, W=4096), dict(depth_type=2),
           dict(fx=0.0), dict(fx=nan), dict(fy=-1.0), dict(scale=0.0), dict(scale=nan), dict(window=-1), dict(window=9), dict(margin=nan),
           dict(margin=inf), dict(margin=-inf), dict(M=-1), dict(M=(1 << 24) + 1)]
    for host in (True, False):
        for kw in bad:
            assert cv(host, **kw) == INVALID, (host, kw)
    keep = np.ones((4,), dtype=np.uint8)
    pose, image = np.ascontiguousarray(np.eye(4)[:3]), np.ones((2, 3), dtype=np.float32)
    assert cv(True, T=pose.ctypes.data, depth=image.ctypes.data, keep=keep.ctypes.data, window=8) == 0
    assert cv(True, M=0, pts=None, keep=None) == 0 and cv(True, H=0, depth=None, keep=keep.ctypes.data) == 0 and keep.all()
    # novelty: c, pts, N, merge, held, keep, stream
    nv = lib.nbk_frame_cloud_novel
    for args in ((None, p, 4, 0.02, None, p, None), (p, None, 4, 0.02, None, p, None), (p, p, 4, 0.02, None, None, None),
                 (p, p, -1, 0.02, None, p, None), (p, p, (1 << 24) + 1, 0.02, None, p, None), (p, p, 4, nan, None, p, None),
                 (p, p, 0, nan, None, p, None)):
        assert nv(*args) == INVALID, args
    # append: store_pts, store_keep, M, new_pts, new_keep, N, counts, slot_of, workspace, workspace_bytes, stream
    wb = lib.nbk_frame_cloud_append_workspace_bytes
    for M, N in ((-1, 4), (4, -1), (0, 4), ((1 << 24) + 1, 4), (4, (1 << 24) + 1), (-(1 << 40), -(1 << 40))):
        assert wb(M, N) < 0, (M, N)
    assert wb(1, 0) > 0 and wb(4099, 257) >= 8 * (17 + 2) + 8 * (17 + 2 + 1) + 4 * 257 and wb(1 << 24, 1 << 24) > 0
    assert wb(4099, 257) % 64 == 0 and wb(4099, 258) >= wb(4099, 257) and wb(1 << 20, 480 * 640) < (1 << 22)
    ap = lib.nbk_frame_cloud_append
    big = 1 << 30
    for args in ((None, p, 4, p, p, 4, p, None, p, big, None), (p, None, 4, p, p, 4, p, None, p, big, None),
                 (p, p, 4, None, p, 4, p, None, p, big, None), (p, p, 4, p, None, 4, p, None, p, big, None),
                 (p, p, 4, p, p, 4, None, None, p, big, None), (p, p, 4, p, p, 4, p, None, None, big, None),
                 (p, p, 0, p, p, 4, p, None, p, big, None), (p, p, -1, p, p, 4, p, None, p, big, None), (p, p, 4, p, p, -1, p, None, p, big, None),
                 (p, p, 4, p, p, 4, p, None, p, wb(4, 4) - 1, None), (p, p, 4, p, p, 4, p, None, p + 8, big, None)):
        assert ap(*args) == INVALID, args
    assert p % 64 == 0 or ap(p, p, 4, p, p, 4, p, None, p, big, None) == INVALID, "a misaligned workspace is refused"


def test_header_and_symbols_agree_on_the_new_names():
    header = open(os.path.join(ROOT, "include", "nbk.h")).read()
    declared = set(re.findall(r"\b(nbk_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(_lib.load(), name), name
    fused = {s for s in declared if s.startswith("nbk_frame_cloud_")}
    assert fused == {s for s in _lib.SYMBOLS if s.startswith("nbk_frame_cloud_")} and set(NEW) <= fused


def test_rendered_scene_is_what_it_says():
    """The analytic scene of the GPU tests: every pixel is the wall or the sphere, the sphere is in every pose's view, and the
    back-projected points lie on the wall plane or on the sphere."""
    H, W = 17, 33
    from numbotics_amd.physics import intrinsics_from_fov
    intr = intrinsics_from_fov(W, H, 50.0)
    for T in fc.POSES:
        assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12
        d = fc.render(T, intr, H, W)
        pts, keep = dc.backproject_ref(d, intr, T)
        assert keep.all()
        on_wall = np.abs(pts[:, 0] - fc.WALL_X) < 1e-6
        on_sphere = np.abs(np.linalg.norm(pts - fc.SPHERE_C, axis=1) - fc.SPHERE_R) < 1e-6
        assert (on_wall | on_sphere).all() and 8 <= on_sphere.sum() <= H * W // 2, (on_wall.sum(), on_sphere.sum())
