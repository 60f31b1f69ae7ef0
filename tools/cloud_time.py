"""Point-cloud obstacles, measured on one GPU (`profiles/cloud_time.log`).

    python tools/cloud_time.py [--out profiles/cloud_time.log] [--append] [--only update,validity,clearance,sweep,baseline,edges,certified,splines,records,depth,fuse,render] [--reps 5]

The c2 arm (its cube plays no part: the cloud entries look at the cloud alone) against the "scan" of tests/cloud_cases.py -- half
the points on a wall x = 0.45, half on a table z = 0.10 -- at N = 1e3 .. 1e6 points of radius 0.01, the base link's shape left out
(it stands on the table: with it every configuration collides and every lane stops at its first cell).  One HIP event pair
around a window of back-to-back calls sized to about 50 ms (the time per call is the window's over its calls, so a call of a few
microseconds is not timed as one launch), a warm-up per shape, the median of --reps windows; the log is written line by line:
    update      PointCloud.update (memset + count + scan + scatter)
    validity    DeviceModel.cloud_validity at B = 1e5 and 1e6, packed words
    clearance   DeviceModel.cloud_clearance at B = 1e5, d_max = 0.05
    sweep       cloud_validity and the update at N = 1e5, B = 1e5 against the cell size (0.0075: 3.5e6 cells, near the 2^22 limit,
                where the update's one-workgroup scan is the longest)
    baseline    N = 1e3: nbk_validity_batch on a descriptor that holds the same points as sphere world shapes with the same pairs
                (the only route without this entry), same process, same q, the windows of the two alternating; the two masks
                must be equal
    edges       DeviceModel.cloud_edge_validity at N = 1e3 and 1e5: E = 1e5 edges from the first configurations, up to 1.0 long, at
                resolution 0.05 and 0.01, max_distance 1.0, connect mode (the lengths are passed as `dist`, so that the rows below
                are the same samples).  Against it, windows alternating: cloud_validity on the same samples written out as q rows
                ahead of time (what had to be done without this entry, less its costs of writing the rows and reducing the mask),
                whose per-edge AND must equal `valid`.  Then, at N = 1e5, the connector's sequence on the c2 scene -- edge_validity,
                then the cloud call ANDed into its result -- next to its two parts alone
    certified   (only when asked for) DeviceModel.cloud_edge_continuous on the c2 scene against scan(100 000) of radius 0.005: E = 1e4
                of the edges above, ContinuousConnector's defaults (max_iter 64, slack 1e-6), at look_ahead 0.02, 0.05, 0.1, 0.2 and
                inf: the time of the cloud call alone and of the connector's sequence (edge_continuous, then the cloud's items reduced
                into its result), with the FREE / COLLISION / UNDECIDED counts of both.  The default look_ahead is the fastest value
                whose UNDECIDED count is no higher than at inf
    splines     (only when asked for) S = 1e3 B-spline trajectories of 8 control points, degree 3 (a random walk of legs 0.05 to 0.25
                long from the first configurations) against the scans of N = 1e3 and 1e5 points: DeviceModel.cloud_spline_validity at
                resolution 0.01 (radius 0.01) per sample, and DeviceModel.cloud_spline_continuous (radius 0.005, max_iter 64, slack
                1e-6) per (trajectory, shape) item at each look_ahead of the certified table; next to each, windows alternating, the
                straight-edge entry on E = 1e3 of the edges above against the same cloud: cloud_edge_validity per sample,
                cloud_edge_continuous per (edge, shape) item
    records     (only when asked for) c2 against scan(100 000), B = 1e5 configurations, d_max = 0.05: DeviceModel.cloud_clearance, then
                DeviceModel.cloud_records per configuration with witness and rows, with the witness alone and with neither, windows
                alternating with the clearance call's; then per (configuration, shape) with rows.  Each line has the ratio to the
                clearance windows it alternated with.  (profiles/cloud_records_time.log)
    depth       (only when asked for) c2 and synthetic float32 frames of 640x480 and 1280x720 pixels from a camera 1.6 m in front of
                the arm, looking along x (vertical field of view 50 degrees): a wall behind the arm, a column of pixels on the arm
                itself at the configuration the frame is taken at, about 15 % holes (zeros).  At least 10 windows each:
                backproject; DeviceModel.cloud_self_filter at the cloud's radius and padding 0.02, every shape (with its grid, and
                beside it the same launch for one workgroup's 256 points: the preamble and the launch, little else);
                PointCloud.update(points, keep); the whole update_from_depth; and PointCloud.update on the surviving points as a
                ready array -- the yardstick.  (profiles/cloud_depth_time.log)
    fuse        (only when asked for) c2 and 640x480 float32 frames of the analytic scene of tests/cloud_fuse_cases.py (a wall and a
                sphere in front of it, rendered by ray casting) from a ring of 8 camera poses around it, integrated into a map of
                capacity 2^20 (radius 0.01, merge distance = the radius, carve margin 0.05, window 1, the arm's filter on the frame
                and on the store).  The ring is integrated twice first (the counts of every call are printed); then, in that steady
                state, at least 10 windows each: PointCloud.integrate_depth cycling over the ring; the prefixes 1, 1..2, ... 1..7 of its
                seven steps on the last frame, a step's time being the difference of two (the steps that write are idempotent there);
                and update_from_depth of the same frame on a cloud of its own.  (profiles/cloud_fuse_time.log)
    render      (only when asked for) c2, the arm and its obstacle drawn, from a camera 1.6 m from the arm (vertical field of view 60
                degrees, defaults otherwise: eps 1e-6, 256 steps): DeviceModel.render_depth of 160x120 and 640x480 frames, B = 1 and
                B = 16 configurations under one pose, at least 10 windows each: ms per frame, distance evaluations per pixel and
                the unresolved share (its counts); beside it, for orientation only, backproject + cloud_self_filter of the frame it
                rendered, windows alternating.  (profiles/cloud_render_time.log)
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from numbotics_amd.engine import DeviceModel  # noqa: E402
from numbotics_amd.physics import PointCloud  # noqa: E402
from numbotics_amd.scenes import build_scene, sample_q  # noqa: E402
from cloud_cases import scan, cloud_model  # noqa: E402

RADIUS = 0.01
BOX = ([-0.6, -0.6, 0.0], [0.6, 0.6, 1.0])
OUT = None


def say(text):
    print(text, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(text + "\n")


def window_calls(fn):
    """Calls per timed window: enough to fill about 50 ms (1 .. 500), from one timed call after a warm-up call."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    t = max(e0.elapsed_time(e1), 1e-3)
    return int(min(500, max(1, round(50.0 / t)))), t


def window(fn, calls):
    """Milliseconds per call of one event pair around `calls` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def summary(out, calls):
    return statistics.median(out), min(out), max(out), calls


def timed(fn, reps):
    """Median / min / max milliseconds per call over `reps` windows of back-to-back calls (window_calls), after a warm-up."""
    calls, t = window_calls(fn)
    reps = max(1, min(reps, int(10000.0 / t)))          # (a call of seconds is not repeated five times)
    return summary([window(fn, calls) for _ in range(reps)], calls)


def timed_pair(fa, fb, reps):
    """The same for two callables, their windows alternating (a b a b ...), so that both see the same machine."""
    ca, cb = window_calls(fa)[0], window_calls(fb)[0]
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(fa, ca))
        tb.append(window(fb, cb))
    return summary(ta, ca), summary(tb, cb)


def fmt(t):
    return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f}; {t[3]} calls/window)"


def edges(q, E, seed, length):
    """E edges from the first rows of q: a random direction, a length drawn from U(0.02, length)."""
    rng = np.random.default_rng(seed); s = q[:E].copy()
    d = rng.standard_normal(s.shape); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return s, s + d * rng.uniform(0.02, length, (E, 1))


def sample_rows(st, gt, d, resolution, ns):
    """The samples of the connect-mode edges st -> gt of lengths d as q rows, by the rule of nbk_edge_validity_batch (step =
    resolution / d, n = ceil(1 / step), t_i = i * step for i < n, t_n = 1; q in three roundings) -> rows, edge of each row."""
    E = st.shape[0]
    step = resolution / d
    n = torch.ceil(1.0 / step).to(torch.int64)
    assert torch.equal(n + 1, ns.to(torch.int64)), "the sample counts restated here differ from the library's"
    offs = torch.cumsum(n + 1, 0) - (n + 1)
    e_of = torch.repeat_interleave(torch.arange(E, device=st.device), n + 1)
    i = torch.arange(e_of.shape[0], device=st.device) - offs[e_of]
    t = torch.where(i < n[e_of], i.to(torch.float64) * step[e_of], torch.ones((), dtype=torch.float64, device=st.device))
    a = (1.0 - t)[:, None] * st[e_of]
    b = t[:, None] * gt[e_of]
    return (a + b).contiguous(), e_of


def edges_part(dev, sm, chain, shapes, reps):
    E = 10 ** 5
    s, g = edges(sample_q(chain, E, seed=1), E, 7, 1.0)
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    d = torch.linalg.norm(gt - st, dim=1)
    say(f"edges: E = {E}, lengths U(0.02, 1.0), max_distance 1.0, connect; workspace {dev.cloud_edge_workspace_bytes(E)} bytes")
    for N in (10 ** 3, 10 ** 5):
        cloud = PointCloud(torch.from_numpy(scan(N, seed=N)).cuda(), RADIUS, bounds=BOX)
        for res in (0.05, 0.01):
            call = lambda: dev.cloud_edge_validity(cloud, st, gt, res, 1.0, dist=d, shapes=shapes)      # noqa: E731
            valid, _, ns = call()
            total = int(ns.sum())
            rows, e_of = sample_rows(st, gt, d, res, ns)
            hit = dev.cloud_validity(cloud, rows, 0.0, shapes=shapes)
            blocked = torch.zeros((E,), dtype=torch.bool, device="cuda")
            blocked[e_of[hit]] = True
            assert torch.equal(valid, ~blocked), "the per-edge AND of the rows' mask differs from cloud_edge_validity"
            te, tr = timed_pair(call, lambda: dev.cloud_validity(cloud, rows, 0.0, packed=True, shapes=shapes), reps)
            say(f"  N = {N:6d} resolution {res}: {total} samples, valid {float(valid.float().mean()):.3f}   edges {fmt(te)}  "
                f"{total / te[0] / 1e6:.2f} G samples/s   rows written out ({rows.numel() * 8 / 1e6:.0f} MB) {fmt(tr)}   "
                f"ratio {tr[0] / te[0]:.2f}x   verdicts equal")
            del rows, e_of, hit
    # the connector's sequence on the c2 scene (its cube rejects part of the edges before the cloud is asked)
    N, res = 10 ** 5, 0.05
    cloud = PointCloud(torch.from_numpy(scan(N, seed=N)).cuda(), RADIUS, bounds=BOX)

    def scene():
        return dev.edge_validity(st, gt, res, 1.0, dist=d)[0]

    def both():
        v = scene()
        dev.cloud_edge_validity(cloud, st, gt, res, 1.0, dist=d, shapes=shapes, out=v)
        return v
    own, full = scene(), both()
    alone = dev.cloud_edge_validity(cloud, st, gt, res, 1.0, dist=d, shapes=shapes)[0]
    assert torch.equal(full, own & alone)
    say(f"  N = {N:6d} resolution {res}, c2 scene: valid {float(own.float().mean()):.3f} after the scene, {float(full.float().mean()):.3f} after both")
    say(f"    edge_validity                          {fmt(timed(scene, reps))}")
    say(f"    cloud_edge_validity alone              {fmt(timed(lambda: dev.cloud_edge_validity(cloud, st, gt, res, 1.0, dist=d, shapes=shapes), reps))}")
    say(f"    edge_validity, cloud_edge_validity(out) {fmt(timed(both, reps))}")


def certified_part(dev, chain, shapes, reps):
    E, N, radius = 10 ** 4, 10 ** 5, 0.005
    s, g = edges(sample_q(chain, E, seed=1), E, 7, 1.0)
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    d = torch.linalg.norm(gt - st, dim=1)
    cloud = PointCloud(torch.from_numpy(scan(N, seed=N)).cuda(), radius, bounds=BOX)
    say(f"certified: E = {E}, lengths U(0.02, 1.0), max_distance 1.0, connect, max_iter 64, slack 1e-6; N = {N}, radius {radius}")
    counts = lambda status: " ".join(f"{name} {int((status == k).sum()):5d}" for k, name in enumerate(("FREE", "COLLISION", "UNDECIDED")))   # noqa: E731
    own = dev.edge_continuous(st, gt, 1.0, dist=d)
    say(f"  edge_continuous alone (the scene)   {fmt(timed(lambda: dev.edge_continuous(st, gt, 1.0, dist=d), reps))}   {counts(own[3])}")
    for la in (0.02, 0.05, 0.1, 0.2, float("inf")):
        alone = lambda: dev.cloud_edge_continuous(cloud, st, gt, 1.0, look_ahead=la, dist=d, shapes=shapes)      # noqa: E731

        def both():
            v, _, tf, status = dev.edge_continuous(st, gt, 1.0, dist=d)
            dev.cloud_edge_continuous(cloud, st, gt, 1.0, look_ahead=la, dist=d, shapes=shapes, out=(v, tf, status))
            return status
        sa, sb = alone()[3], both()
        say(f"  look_ahead {la:5.2f}: cloud alone {fmt(timed(alone, reps))}   {counts(sa)}")
        say(f"                    scene + cloud {fmt(timed(both, reps))}   {counts(sb)}")


def splines_part(dev, chain, shapes, reps):
    from numbotics_amd.planning import unit_knots
    S, n, k, res = 10 ** 3, 8, 3, 0.01
    q = sample_q(chain, S, seed=1)
    rng = np.random.default_rng(11)
    legs = rng.standard_normal((S, n - 1, q.shape[1]))
    legs *= rng.uniform(0.05, 0.25, (S, n - 1, 1)) / np.linalg.norm(legs, axis=2, keepdims=True)
    ct = torch.from_numpy(np.concatenate((q[:, None], q[:, None] + np.cumsum(legs, axis=1)), axis=1)).cuda()
    kn = torch.from_numpy(unit_knots(n, k)).cuda()
    s, g = edges(q, S, 7, 1.0)
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    d = torch.linalg.norm(gt - st, dim=1)
    K = len(shapes)
    say(f"splines: S = {S} trajectories of {n} control points, degree {k}; edges: E = {S}, lengths U(0.02, 1.0), connect; {K} shapes")
    for N in (10 ** 3, 10 ** 5):
        cloud = PointCloud(torch.from_numpy(scan(N, seed=N)).cuda(), RADIUS, bounds=BOX)
        spl = lambda: dev.cloud_spline_validity(cloud, ct, kn, k, res, shapes=shapes)                     # noqa: E731
        edg = lambda: dev.cloud_edge_validity(cloud, st, gt, res, 1.0, dist=d, shapes=shapes)              # noqa: E731
        (v, _, ns), (ve, _, nse) = spl(), edg()
        ts, te = timed_pair(spl, edg, reps)
        say(f"  sampled   N = {N:6d} resolution {res}: splines {int(ns.sum())} samples, valid {float(v.float().mean()):.3f}  {fmt(ts)}  "
            f"{ts[0] * 1e6 / int(ns.sum()):.2f} ns/sample   edges {int(nse.sum())} samples, valid {float(ve.float().mean()):.3f}  {fmt(te)}  "
            f"{te[0] * 1e6 / int(nse.sum()):.2f} ns/sample")
    counts = lambda status: " ".join(f"{name} {int((status == j).sum()):4d}" for j, name in enumerate(("FREE", "COLLISION", "UNDECIDED")))   # noqa: E731
    for N in (10 ** 3, 10 ** 5):
        cloud = PointCloud(torch.from_numpy(scan(N, seed=N)).cuda(), 0.005, bounds=BOX)
        for la in (0.02, 0.05, 0.1, 0.2, float("inf")):
            spl = lambda: dev.cloud_spline_continuous(cloud, ct, kn, k, look_ahead=la, shapes=shapes)      # noqa: E731
            edg = lambda: dev.cloud_edge_continuous(cloud, st, gt, 1.0, look_ahead=la, dist=d, shapes=shapes)   # noqa: E731
            ss, se = spl()[2], edg()[3]
            ts, te = timed_pair(spl, edg, reps)
            say(f"  certified N = {N:6d} radius 0.005 look_ahead {la:5.2f}: splines {fmt(ts)}  {ts[0] * 1e3 / (S * K):.2f} us/item  {counts(ss)}   "
                f"edges {fmt(te)}  {te[0] * 1e3 / (S * K):.2f} us/item  {counts(se)}")


def records_part(dev, sm, shapes, q5, reps):
    N, d_max = 10 ** 5, 0.05
    cloud = PointCloud(torch.from_numpy(scan(N, seed=N)).cuda(), RADIUS, bounds=BOX)
    clr = lambda: dev.cloud_clearance(cloud, q5, d_max, shapes=shapes)                                  # noqa: E731
    d, s, p = clr()
    near = torch.isfinite(d)
    say(f"records: N = {N}, B = {q5.shape[0]}, d_max {d_max}, {len(shapes)} shapes; below d_max {float(near.float().mean()):.3f}")
    say(f"  cloud_clearance alone                    {fmt(timed(clr, reps))}")
    for name, kw in (("per configuration, witness + rows", {}), ("per configuration, witness", dict(jacobian=False)),
                     ("per configuration, neither", dict(witness=False, jacobian=False)), ("per shape, witness + rows", dict(per_shape=True))):
        rec = lambda: dev.cloud_records(cloud, q5, d_max, shapes=shapes, **kw)                          # noqa: E731
        r = rec()
        if not kw.get("per_shape"):
            assert torch.equal(r[0][near], d[near]) and torch.equal(r[1], s) and torch.equal(r[2], p), "records and clearance differ"
            share = ""
        else:
            share = f"   items below d_max {float(torch.isfinite(r[0]).float().mean()):.3f}"
        tr, tc = timed_pair(rec, clr, reps)
        say(f"  {name:36s} {fmt(tr)}   clearance beside it {fmt(tc)}   ratio {tr[0] / tc[0]:.2f}x{share}")


def depth_part(arm, dev, sm, chain, reps):
    from numbotics_amd.physics import backproject, intrinsics_from_fov
    reps = max(reps, 10)
    pad = 0.02
    q0 = sample_q(chain, 4, seed=5)[2]
    qt = torch.from_numpy(q0).cuda()
    cam = np.array([[1.0, 0.0, 0.0, -1.6], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.55], [0.0, 0.0, 0.0, 1.0]])
    Tt = torch.from_numpy(cam).cuda()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    say(f"depth: c2 ({sm.n_rshapes} shapes, all filtered), radius {RADIUS}, padding {pad}, camera at (-1.6, 0, 0.55) looking along x; {cus} CUs; >= {reps} windows")
    for W, H in ((640, 480), (1280, 720)):
        rng = np.random.default_rng(W)
        intr = intrinsics_from_fov(W, H, 50.0)
        u, v = np.meshgrid(np.arange(W), np.arange(H))
        z = np.full((H, W), 2.05) + rng.uniform(-0.01, 0.01, (H, W))                 # the wall
        col = np.abs((u - intr[2]) / intr[0]) < 0.06                                   # the arm's column: 0.1 m either side at 1.6 m
        z[col] = 1.6 + rng.uniform(-0.06, 0.06, int(col.sum()))
        z[rng.uniform(size=(H, W)) < 0.15] = 0.0
        dt = torch.from_numpy(z.astype(np.float32)).cuda()
        n = H * W
        pts, keep = backproject(dt, intr, Tt, frame="numbotics")
        valid = int(keep.sum())
        lo, hi = pts[keep.bool()].min(0).values.cpu().numpy(), pts[keep.bool()].max(0).values.cpu().numpy()
        cloud = PointCloud(np.zeros((0, 3)), RADIUS, bounds=(lo, hi), capacity=n)
        k2 = keep.clone()
        dev.cloud_self_filter(pts, qt, RADIUS, pad, keep=k2)
        left = int(k2.sum())
        surv = pts[k2.bool()].contiguous()
        grid = min((n + 255) // 256, 4 * cus)
        say(f"  {W}x{H}: {n} pixels, {valid} valid ({1 - valid / n:.3f} holes), the filter removes {valid - left} ({(valid - left) / valid:.3f}); "
            f"cell {cloud.cell:.4f}, grid {tuple(int(d) for d in cloud.dims)}; filter grid {grid} workgroups of 256")
        say(f"    backproject                         {fmt(timed(lambda: backproject(dt, intr, Tt, frame='numbotics', out=(pts, keep)), reps))}")

        def filt():
            k2.copy_(keep)
            dev.cloud_self_filter(pts, qt, RADIUS, pad, keep=k2)
        say(f"    self-filter (with the mask's copy)  {fmt(timed(filt, reps))}")
        say(f"    the mask's copy alone               {fmt(timed(lambda: k2.copy_(keep), reps))}")
        k1, p1 = torch.ones((256,), dtype=torch.uint8, device='cuda'), pts[:256].contiguous()
        say(f"    self-filter, 256 points (1 workgroup) {fmt(timed(lambda: dev.cloud_self_filter(p1, qt, RADIUS, pad, keep=k1), reps))}")
        say(f"    update(points, keep)                {fmt(timed(lambda: cloud.update(pts, keep=k2), reps))}")
        say(f"    update_from_depth, all three        {fmt(timed(lambda: cloud.update_from_depth(dt, intr, Tt, arm=arm, q=qt, padding=pad, frame='numbotics'), reps))}")
        assert cloud.count() == left
        say(f"    update({left} surviving points)      {fmt(timed(lambda: cloud.update(surv), reps))}")
        say(f"    update(all {n} pixels, no mask)     {fmt(timed(lambda: cloud.update(pts), reps))}")


def render_part(arm, dev, sm, chain, reps):
    from numbotics_amd.physics import backproject, intrinsics_from_fov
    reps = max(reps, 10)
    pad = 0.02
    qs = sample_q(chain, 16, seed=5)
    cam = np.array([[-1.0, 0.0, 0.0, 1.6], [0.0, -1.0, 0.0, 0.3], [0.0, 0.0, 1.0, 0.6], [0.0, 0.0, 0.0, 1.0]])
    Tt = torch.from_numpy(cam).cuda()
    cnt = torch.zeros((3,), dtype=torch.int64, device="cuda")
    say(f"render: c2 ({sm.n_rshapes} robot shapes, {sm.n_wshapes} world), camera at (1.6, 0.3, 0.6) looking along -x, fov 60, near 0.01, far 1000, "
        f"eps 1e-6, max_steps 256; >= {reps} windows")
    for W, H in ((160, 120), (640, 480)):
        intr = intrinsics_from_fov(W, H, 60.0)
        for B in (1, 16):
            qt = torch.from_numpy(np.ascontiguousarray(qs[:B])).cuda()
            depth = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
            dev.render_depth(qt, Tt, intr, H, W, out=depth, counts=cnt, frame="numbotics")
            c = cnt.cpu().numpy()
            n = B * H * W
            pts = torch.empty((H * W, 3), dtype=torch.float64, device="cuda")
            keep = torch.empty((H * W,), dtype=torch.uint8, device="cuda")

            def consume():
                backproject(depth[0], intr, Tt, frame="numbotics", out=(pts, keep))
                dev.cloud_self_filter(pts, qt[0], RADIUS, pad, keep=keep)
            tr, tc = timed_pair(lambda: dev.render_depth(qt, Tt, intr, H, W, out=depth, frame="numbotics"), consume, reps)
            say(f"  {W}x{H} B = {B:2d}: render {fmt(tr)} = {tr[0] / B:.3f} ms/frame; hit {c[0] / n:.3f}, unresolved {c[1] / n:.5f}, "
                f"{c[2] / n:.2f} distance evaluations/pixel")
            say(f"           backproject + self-filter of frame 0 (padding {pad}) {fmt(tc)}")


def fuse_part(arm, dev, sm, chain, reps):
    from numbotics_amd.physics import backproject, intrinsics_from_fov
    from numbotics_amd.physics.pointcloud import append, carve
    import cloud_fuse_cases as fc
    reps = max(reps, 10)
    W, H, cap, pad, margin, window = 640, 480, 1 << 20, 0.02, 0.05, 1
    intr = intrinsics_from_fov(W, H, 50.0)
    q0 = sample_q(chain, 4, seed=5)[2]
    qt = torch.from_numpy(q0).cuda()
    centre = np.array([0.3, 0.0, 0.5])
    poses = []
    for k in range(8):
        a = -0.6 + 1.2 * k / 7.0                                                     # the ring: an arc of 1.7 m around the scene
        pos = centre + 1.7 * np.array([-np.cos(a), np.sin(a), 0.0]) + [0.0, 0.0, 0.1 * (k % 3 - 1)]
        poses.append(fc.look_along_x(pos, yaw=-a, pitch=0.06 * (k % 3 - 1)))
    frames = [torch.from_numpy(fc.render(T, intr, H, W)).cuda() for T in poses]
    Ts = [torch.from_numpy(np.ascontiguousarray(T)).cuda() for T in poses]
    box = ([-0.1, -3.2, -1.3], [0.7, 3.2, 2.5])                                       # what the eight frames see of the wall
    cloud = PointCloud(np.zeros((0, 3)), RADIUS, bounds=box, capacity=cap)
    kw = dict(arm=arm, q=qt, padding=pad, carve_margin=margin, carve_window=window)
    say(f"fuse: c2 ({sm.n_rshapes} shapes, all filtered), {W}x{H} float32 frames, ring of {len(poses)} poses, capacity {cap}, radius = merge {RADIUS}, "
        f"carve margin {margin} window {window}, padding {pad}; cell {cloud.cell:.4f}, grid {tuple(int(d) for d in cloud.dims)}; >= {reps} windows")
    for lap in range(2):
        for k in range(len(poses)):
            cloud.integrate_depth(frames[k], intr, Ts[k], **kw)
            say(f"  lap {lap} pose {k}: {cloud.map_counts()}")
    ring = [0]

    def whole():
        k = ring[0] = (ring[0] + 1) % len(poses)
        cloud.integrate_depth(frames[k], intr, Ts[k], **kw)
    say(f"    integrate_depth, over the ring      {fmt(timed(whole, reps))}")
    k = len(poses) - 1
    sp, sk = cloud.integrate_depth(frames[k], intr, Ts[k], **kw)
    say(f"    steady state at the last pose: {cloud.map_counts()}")
    say(f"    integrate_depth, the last frame     {fmt(timed(lambda: cloud.integrate_depth(frames[k], intr, Ts[k], **kw), reps))}")
    mp = cloud._map
    pts, keep = cloud._stage.pts, cloud._stage.keep
    # a step's time is the difference of two prefixes of the sequence: each prefix starts from the back-projection, so that the
    # frame's mask is the one the step sees inside the call (alone, after the call, steps 2 and 5 would find it all zeros)
    def prefix(n):
        backproject(frames[k], intr, Ts[k], out=(pts, keep))
        if n >= 2:
            dev.cloud_self_filter(pts, qt, RADIUS, pad, keep=keep)
        if n >= 3:
            carve(sp, sk, frames[k], intr, Ts[k], margin, window)
        if n >= 4:
            dev.cloud_self_filter(sp, qt, RADIUS, pad, keep=sk)
        if n >= 5:
            cloud.novel(pts, keep, RADIUS, held=sk)
        if n >= 6:
            append(sp, sk, pts, keep, counts=mp.counts, workspace=mp.ws)
        if n >= 7:
            cloud.update(sp, keep=sk)
    before = 0.0
    for n, name in enumerate(("backproject", "self-filter, the frame", "carve", "self-filter, the store", "novel", "append",
                              f"update(store, keep), N = {cap}"), 1):
        t = timed(lambda: prefix(n), reps)
        say(f"    steps 1..{n} {fmt(t)}   step {n}, {name}: {t[0] - before:.3f} ms")
        before = t[0]
    held = cloud.count()
    one = PointCloud(np.zeros((0, 3)), RADIUS, bounds=box, capacity=H * W)
    say(f"    update_from_depth, the same frame   {fmt(timed(lambda: one.update_from_depth(frames[k], intr, Ts[k], arm=arm, q=qt, padding=pad), reps))}")
    say(f"    the map holds {held} points, the single frame's cloud {one.count()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out instead of starting it anew")
    ap.add_argument("--only", default="update,validity,clearance,sweep,baseline,edges")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-n", type=int, default=10 ** 6)
    a = ap.parse_args()
    only = set(a.only.split(","))
    global OUT
    OUT = a.out
    if OUT:
        open(OUT, "a" if a.append else "w").close()
    if not torch.cuda.is_available():
        raise SystemExit("cloud_time.py measures on the GPU: none visible")
    arm, chain, obs = build_scene("c2")
    sm = arm.scene_model()
    dev = DeviceModel(sm)
    shapes = list(range(1, sm.n_rshapes))
    from numbotics_amd.csrc.build import source_digest
    say(f"# cloud_time.py  kernels {source_digest()}  device {torch.cuda.get_device_name(0)}  robot c2 ({sm.n_rshapes} shapes, base left out)  radius {RADIUS}")
    q5 = torch.from_numpy(sample_q(chain, 10 ** 5, seed=1)).cuda()
    q6 = torch.from_numpy(sample_q(chain, 10 ** 6, seed=2)).cuda()
    sizes = [n for n in (10 ** 3, 10 ** 4, 10 ** 5, 10 ** 6) if n <= a.max_n] if only & {"update", "validity", "clearance"} else []
    for N in sizes:
        pts = torch.from_numpy(scan(N, seed=N)).cuda()
        cloud = PointCloud(pts, RADIUS, bounds=BOX)
        say(f"N = {N}: cell {cloud.cell:.4f}, grid {tuple(int(d) for d in cloud.dims)}")
        if "update" in only:
            say(f"  update                      {fmt(timed(lambda: cloud.update(pts), a.reps))}")
        if "validity" in only:
            frac = float(dev.cloud_validity(cloud, q5, 0.0, shapes=shapes).float().mean())
            say(f"  validity  B = 1e5           {fmt(timed(lambda: dev.cloud_validity(cloud, q5, 0.0, packed=True, shapes=shapes), a.reps))}   colliding {frac:.3f}")
            say(f"  validity  B = 1e6           {fmt(timed(lambda: dev.cloud_validity(cloud, q6, 0.0, packed=True, shapes=shapes), a.reps))}")
        if "clearance" in only:
            d, _, _ = dev.cloud_clearance(cloud, q5, 0.05, shapes=shapes)
            say(f"  clearance B = 1e5 d_max .05 {fmt(timed(lambda: dev.cloud_clearance(cloud, q5, 0.05, shapes=shapes), a.reps))}   below d_max {float(torch.isfinite(d).float().mean()):.3f}")
    if "sweep" in only and 10 ** 5 <= a.max_n:
        N = 10 ** 5
        pts = torch.from_numpy(scan(N, seed=N)).cuda()
        say(f"cell sweep: validity at N = {N}, B = 1e5")
        ref = None
        for cell in (0.0075, 0.0125, 0.02, 0.03, 0.05, 0.075, 0.1, 0.15, 0.25, 0.5):
            cloud = PointCloud(pts, RADIUS, cell=cell, bounds=BOX)
            m = dev.cloud_validity(cloud, q5, 0.0, packed=True, shapes=shapes)
            if ref is None:
                ref = m
            assert torch.equal(m, ref), "the cell size changed a result"
            say(f"  cell {cell:6.4f} grid {str(tuple(int(d) for d in cloud.dims)):>15}  {fmt(timed(lambda: dev.cloud_validity(cloud, q5, 0.0, packed=True, shapes=shapes), a.reps))}"
                f"   update {fmt(timed(lambda: cloud.update(pts), a.reps))}")
    if "baseline" in only:
        N = 10 ** 3
        host_pts = scan(N, seed=N)
        cloud = PointCloud(host_pts, RADIUS, bounds=BOX)
        base = DeviceModel(cloud_model(sm, host_pts, RADIUS, shapes))
        say(f"baseline at N = {N}: the same points as {N} sphere world shapes, {base.n_pairs} pairs, nbk_validity_batch")
        for name, q in (("1e5", q5), ("1e6", q6)):
            mc = dev.cloud_validity(cloud, q, 0.0, packed=True, shapes=shapes)
            mb = base.validity(q, 0.0, packed=True)
            assert torch.equal(mc, mb), "cloud and sphere-descriptor masks differ"
            tc, tb = timed_pair(lambda: dev.cloud_validity(cloud, q, 0.0, packed=True, shapes=shapes),
                                lambda: base.validity(q, 0.0, packed=True), a.reps)
            say(f"  B = {name}: cloud {fmt(tc)}   sphere descriptor {fmt(tb)}   ratio {tb[0] / tc[0]:.2f}x   masks equal")
    if "edges" in only:
        edges_part(dev, sm, chain, shapes, a.reps)
    if "certified" in only:
        certified_part(dev, chain, shapes, a.reps)
    if "splines" in only:
        splines_part(dev, chain, shapes, a.reps)
    if "records" in only:
        records_part(dev, sm, shapes, q5, a.reps)
    if "depth" in only:
        depth_part(arm, dev, sm, chain, a.reps)
    if "fuse" in only:
        fuse_part(arm, dev, sm, chain, a.reps)
    if "render" in only:
        render_part(arm, dev, sm, chain, a.reps)


if __name__ == "__main__":
    main()
