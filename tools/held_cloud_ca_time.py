"""Certified edges and splines of the held object against a point cloud, measured on one GPU ("Held objects").

    python tools/held_cloud_ca_time.py [--out profiles/held_cloud_ca_time.log] [--look-ahead 0.05]

Scene c2 with the box of the parity fixtures in the hand (half extents 0.1, 0.1, 0.2, margin 0.04, 0.25 m along the gripper's z;
H = 1), against the dense scan at 1e5 points (scan(N, seed=N), radius 0.01, the box of tools/cloud_time.py).  One HIP event pair
around each call, 3 warm-up runs, the median of 20 timed runs; connect mode, threshold 0, max_iter 64, slack 1e-6, look_ahead 0.05
for the two entries that take one (with look_ahead inf the first step of an edge this long walks all 1e5 points in every lane:
DESIGN.md section 6 has 4.4 s per call for the arm on edges a third as long, and 23 such calls per line are not a measurement
anyone waits for).
    edges     E = 1e4 edges of bench.py's edge distribution (end points U(limits), |dq| <= pi = max_distance, rng seed 3):
              DeviceModel.held_cloud_edge_continuous alone, and in the same run DeviceModel.cloud_edge_continuous (the arm's shapes
              off the base link) and DeviceModel.held_edge_continuous as the yardsticks.
    splines   S = 1e3 cubic trajectories of 8 control points (the legs of tools/cloud_time.py's splines: lengths U(0.05, 0.25)):
              the three spline entries the same way.
The statuses each call reports are printed beside its time: the three calls ask different questions of the same trajectories.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cloud_time import scan, RADIUS, BOX                                         # noqa: E402
from numbotics_amd.csrc.build import source_digest                               # noqa: E402
from numbotics_amd.physics import Cuboid, PointCloud                             # noqa: E402
from numbotics_amd.planning import unit_knots                                    # noqa: E402
from numbotics_amd.scenes import build_scene, sample_q                           # noqa: E402

WARM, RUNS = 3, 20


def timed(fn):
    """Median / min / max milliseconds of RUNS calls, one HIP event pair each, after WARM calls."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def fmt(t):
    return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def shares(status):
    st = status.cpu().numpy()
    return "FREE %d, COLLISION %d, UNDECIDED %d, DEGENERATE %d" % tuple(int((st == k).sum()) for k in range(4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "held_cloud_ca_time.log"))
    ap.add_argument("--look-ahead", type=float, default=0.05)
    args = ap.parse_args()
    la = args.look_ahead
    if not torch.cuda.is_available():
        raise SystemExit("tools/held_cloud_ca_time.py needs a GPU: nothing is measured without one")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    arm, chain, obs = build_scene("c2")
    box = Cuboid(0.0, np.array([0.1, 0.1, 0.2]), collision_margin=0.04, position=np.array([0.0, 0.0, -6.0]))
    G = np.eye(4)
    G[2, 3] = 0.25
    att = arm.attach(box, "gripper", pose=G)
    sm = arm.scene_model()
    dev, held = att._device(arm)
    base = sm.links[sm.rshape_link[0]]._name
    shapes = [k for k in range(sm.n_rshapes) if sm.links[sm.rshape_link[k]]._name != base]
    N, E, S = 10 ** 5, 10 ** 4, 10 ** 3
    cloud = PointCloud(torch.from_numpy(scan(N, seed=N)).cuda(), RADIUS, bounds=BOX)
    say(f"# tools/held_cloud_ca_time.py  build {source_digest()}  {torch.cuda.get_device_name(0)}  N {N}  radius {RADIUS}  "
        f"look_ahead {la}  warm-up {WARM}  runs {RUNS}")
    # ---- edges: bench.py's distribution
    lim = np.asarray(chain.joint_limits, dtype=np.float64)
    rng = np.random.default_rng(3)
    s = rng.uniform(lim[:, 0], lim[:, 1], (E, chain.dof))
    g = rng.uniform(lim[:, 0], lim[:, 1], (E, chain.dof))
    d = np.linalg.norm(g - s, axis=1)
    g = s + (g - s) * np.minimum(1.0, rng.uniform(0.2, 1.0, E) * np.pi / d)[:, None]
    st, gt = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    say(f"## edges: E = {E}, end points U(limits), |dq| <= pi, max_distance pi, connect")
    calls = (("held_cloud_edge_continuous", lambda: dev.held_cloud_edge_continuous(held, cloud, st, gt, np.pi, look_ahead=la)),
             ("cloud_edge_continuous, the arm", lambda: dev.cloud_edge_continuous(cloud, st, gt, np.pi, look_ahead=la, shapes=shapes)),
             ("held_edge_continuous", lambda: dev.held_edge_continuous(held, st, gt, np.pi)))
    t = {}
    for name, fn in calls:
        t[name] = timed(fn)
        say(f"  {name:34s} {fmt(t[name])}   {shares(fn()[3])}")
    say(f"  ratio held_cloud / cloud           {t[calls[0][0]][0] / t[calls[1][0]][0]:9.2f}")
    say(f"  ratio held_cloud / held            {t[calls[0][0]][0] / t[calls[2][0]][0]:9.2f}")
    # ---- cubic splines
    n, k = 8, 3
    q = sample_q(chain, S, seed=1)
    rng = np.random.default_rng(11)
    legs = rng.standard_normal((S, n - 1, q.shape[1]))
    legs *= rng.uniform(0.05, 0.25, (S, n - 1, 1)) / np.linalg.norm(legs, axis=2, keepdims=True)
    ctrl = np.concatenate((q[:, None, :], q[:, None, :] + np.cumsum(legs, axis=1)), axis=1)
    ct = torch.from_numpy(np.ascontiguousarray(ctrl)).cuda()
    knots = unit_knots(n, k)
    say(f"## splines: S = {S}, degree {k}, {n} control points, legs U(0.05, 0.25)")
    calls = (("held_cloud_spline_continuous", lambda: dev.held_cloud_spline_continuous(held, cloud, ct, knots, k, look_ahead=la)),
             ("cloud_spline_continuous, the arm", lambda: dev.cloud_spline_continuous(cloud, ct, knots, k, look_ahead=la, shapes=shapes)),
             ("held_spline_continuous", lambda: dev.held_spline_continuous(held, ct, knots, k)))
    t = {}
    for name, fn in calls:
        t[name] = timed(fn)
        say(f"  {name:34s} {fmt(t[name])}   {shares(fn()[2])}")
    say(f"  ratio held_cloud / cloud           {t[calls[0][0]][0] / t[calls[1][0]][0]:9.2f}")
    say(f"  ratio held_cloud / held            {t[calls[0][0]][0] / t[calls[2][0]][0]:9.2f}")
    log.close()
    del obs, box


if __name__ == "__main__":
    main()
