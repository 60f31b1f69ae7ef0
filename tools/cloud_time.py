"""Point-cloud obstacles, measured on one GPU (`profiles/cloud_time.log`).

    python tools/cloud_time.py [--out profiles/cloud_time.log] [--only update,validity,clearance,sweep,baseline] [--reps 5]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="update,validity,clearance,sweep,baseline")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-n", type=int, default=10 ** 6)
    a = ap.parse_args()
    only = set(a.only.split(","))
    global OUT
    OUT = a.out
    if OUT:
        open(OUT, "w").close()
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
    sizes = [n for n in (10 ** 3, 10 ** 4, 10 ** 5, 10 ** 6) if n <= a.max_n]
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


if __name__ == "__main__":
    main()
